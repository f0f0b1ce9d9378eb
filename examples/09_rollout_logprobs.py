"""RL rollouts with behaviour-policy log-probs: the engine samples with
per-request seeds and reports, for every generated token, its
log-probability under the distribution it was drawn from, its rank and the
most likely alternatives. A policy-gradient step needs exactly these
numbers next to the tokens; a seeded request repeats both, alone or batched.

Run: PYTHONPATH=. python examples/09_rollout_logprobs.py   (CPU or GPU)
"""
import torch

from kubetorch_amd.models import BatchedGenerator, Llama, llama_tiny


def rollout(model, prompts, seeds, n_alt=3, new=8, **engine_kw):
    eng = BatchedGenerator(model, max_batch=4, max_len=64, kv="paged",
                           sampler="fused", logprobs=n_alt, **engine_kw)
    # top_k / top_p stay off: the log-prob is then exactly that of the
    # distribution the token was drawn from (the filters are not applied
    # to the reported distribution)
    rids = [eng.submit(p, max_new_tokens=new, temperature=1.0, seed=s,
                       logprobs=n_alt) for p, s in zip(prompts, seeds)]
    out = eng.run()
    # the caller pops the records; the engine keeps only the latest 4096
    return [(out[r], eng.logprobs.pop(r)) for r in rids]


if __name__ == "__main__":
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    torch.manual_seed(0)
    model = Llama(llama_tiny()).to(dev).eval()
    if dev == "cuda":
        model = model.bfloat16()
    prompts = [[1, 2, 3, 4], [9, 8, 7], [5, 5]]
    runs = rollout(model, prompts, seeds=[11, 12, 13])
    for prompt, (toks, rec) in zip(prompts, runs):
        print("prompt", prompt, "->", rec["tokens"])
        print("  logprobs", [round(v, 3) for v in rec["logprobs"]])
        print("  ranks   ", rec["ranks"])
        print("  top-3 of the first token",
              list(zip(rec["top_ids"][0],
                       [round(v, 3) for v in rec["top_logprobs"][0]])))
        print("  sequence log-prob", round(sum(rec["logprobs"]), 3))
    # the same seed alone gives the same tokens and the same numbers
    again = rollout(model, prompts[1:2], seeds=[12])[0]
    assert again[0] == runs[1][0] and again[1]["ranks"] == runs[1][1]["ranks"]
    print("request 1 alone repeats its rollout:", again[1]["tokens"])
