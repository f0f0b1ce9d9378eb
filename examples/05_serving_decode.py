"""Serve Llama decode as a kubetorch_amd service: KV-cache generation on
one MI355X pod, weights fanned out to replicas through the filesystem
tree broadcast (the store uploads once; pods feed each other).

Run: python examples/05_serving_decode.py   (local driver — no cluster)
"""
import kubetorch_amd as kt


class Generator:
    """Deployed as a kt.cls service: loads weights once, serves decode."""

    def __init__(self, weights_key=None):
        import torch

        from kubetorch_amd.models import Llama, llama_tiny

        dev = "cuda" if torch.cuda.is_available() else "cpu"
        self.model = Llama(llama_tiny()).to(dev).eval()
        if dev == "cuda":
            self.model = self.model.bfloat16()
        if weights_key:
            # replicas join the rolling tree: O(1) store egress at any W
            path = kt.get_broadcast(weights_key, dest="/tmp/weights")
            sd = torch.load(f"{path}/model.pt", map_location=dev)
            self.model.load_state_dict(sd)
        self.device = dev

    def generate(self, prompt_ids, max_new_tokens=16, temperature=0.0):
        import torch

        toks = torch.tensor([prompt_ids], device=self.device)
        out = self.model.generate(toks, max_new_tokens,
                                  temperature=temperature)
        return out[0].tolist()

    def generate_batch(self, prompts, max_new_tokens=16, kv_dtype=None,
                       sampling=None):
        """Continuous batching over the paged KV cache. kv_dtype="fp8"
        keeps the pages as e4m3 bytes (half the KV memory and decode
        reads), with scales calibrated on the first prompt. `sampling`:
        per-prompt dicts of submit()'s temperature / top_k / top_p / seed,
        drawn by the fused sampler; a seeded request repeats its tokens
        whatever it is batched with."""
        from kubetorch_amd.models import BatchedGenerator, calibrate_kv_scales

        scales = None
        if kv_dtype == "fp8":
            scales = calibrate_kv_scales(self.model, prompts[0], margin=1.5)
        eng = BatchedGenerator(self.model, max_batch=4, max_len=128,
                               kv="paged", kv_dtype=kv_dtype,
                               kv_scales=scales,
                               sampler="fused" if sampling else "torch")
        sampling = sampling or [{}] * len(prompts)
        rids = [eng.submit(p, max_new_tokens=max_new_tokens, **s)
                for p, s in zip(prompts, sampling)]
        out = eng.run()
        return [out[r] for r in rids]


if __name__ == "__main__":
    gen = kt.cls(Generator).to(kt.Compute(gpus=0))  # gpus=1 on a cluster
    try:
        ids = gen.generate([1, 2, 3, 4], max_new_tokens=8)
        print("generated:", ids)
        outs = gen.generate_batch([[1, 2, 3, 4], [9, 8, 7]], max_new_tokens=8,
                                  kv_dtype="fp8")
        print("generated (paged fp8 KV):", outs)
        outs = gen.generate_batch(
            [[1, 2, 3, 4], [9, 8, 7]], max_new_tokens=8,
            sampling=[dict(temperature=0.8, top_k=50, top_p=0.9, seed=1234),
                      dict()])  # the second request stays greedy
        print("generated (sampled, seed 1234 / greedy):", outs)
    finally:
        gen.teardown()
