"""Tests for the flagship Llama model and the FlatDDP training engine."""
import os

import pytest
import torch

from kubetorch_amd.models import Llama, llama_tiny
from kubetorch_amd.parallel import FlatDDP
from test_model_float64 import assert_logits_rule, logits_references


def _tiny_model(device="cpu"):
    torch.manual_seed(0)
    cfg = llama_tiny()
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with torch.device(device):
            model = Llama(cfg)
    finally:
        torch.set_default_dtype(prev)
    return model, cfg


def test_forward_shapes():
    model, cfg = _tiny_model()
    x = torch.randint(0, cfg.vocab_size, (2, 32))
    logits = model(x)
    assert logits.shape == (2, 32, cfg.vocab_size)
    assert logits.dtype == torch.bfloat16
    assert model.rope_cos.dtype == torch.float32


def test_loss_decreases_cpu():
    model, cfg = _tiny_model()
    eng = FlatDDP(model, lr=1e-3, bucket_mb=1)
    x = torch.randint(0, cfg.vocab_size, (2, 64))
    y = torch.randint(0, cfg.vocab_size, (2, 64))
    losses = []
    for _ in range(4):
        loss = model.loss(x, y)
        loss.backward()
        eng.step()
        losses.append(loss.item())
    assert losses[-1] < losses[0], losses
    assert all(l == l for l in losses), f"NaN in {losses}"


def test_flatddp_grads_match_autograd():
    """FlatDDP's flat grad views must hold exactly what autograd computes."""
    torch.manual_seed(0)
    model, cfg = _tiny_model()
    x = torch.randint(0, cfg.vocab_size, (1, 32))
    y = torch.randint(0, cfg.vocab_size, (1, 32))

    # plain autograd reference on an identical model
    torch.manual_seed(0)
    ref_model, _ = _tiny_model()
    for p, q in zip(model.parameters(), ref_model.parameters()):
        assert torch.equal(p.data, q.data)

    eng = FlatDDP(model, lr=1e-3, bucket_mb=1)
    torch.manual_seed(42)
    model.loss(x, y).backward()
    torch.manual_seed(42)
    ref_model.loss(x, y).backward()
    for p, q in zip(model.parameters(), ref_model.parameters()):
        # copy-mode: grads live in the flat buckets (p.grad released)
        torch.testing.assert_close(eng._param_view[p], q.grad,
                                   rtol=1e-2, atol=1e-2)

    # view-mode (grad accumulation) keeps p.grad pinned to the bucket
    torch.manual_seed(0)
    model2, _ = _tiny_model()
    eng2 = FlatDDP(model2, lr=1e-3, bucket_mb=1, grad_accum_steps=2)
    torch.manual_seed(42)
    model2.loss(x, y).backward()
    torch.manual_seed(42)
    model2.loss(x, y).backward()
    for p, q in zip(model2.parameters(), ref_model.parameters()):
        torch.testing.assert_close(p.grad, 2 * q.grad, rtol=2e-2, atol=2e-2)


@pytest.mark.gpu
def test_loss_step_gpu():
    model, cfg = _tiny_model("cuda")
    eng = FlatDDP(model, lr=1e-3, bucket_mb=4)
    x = torch.randint(0, cfg.vocab_size, (2, 64), device="cuda")
    y = torch.randint(0, cfg.vocab_size, (2, 64), device="cuda")
    l0 = None
    for _ in range(4):
        loss = model.loss(x, y)
        loss.backward()
        eng.step()
        if l0 is None:
            l0 = loss.item()
    assert loss.item() < l0


@pytest.mark.gpu
def test_gpu_forward_matches_cpu():
    """GPU model (HIP kernels) vs the same weights on CPU (fp32 reference
    path), and vs the float64 reference of test_model_float64.py under its
    logits rule: every row at most as far from float64 as the naive bf16
    composition's worst row, the whole tensor no noisier and no more biased.

    The assert_close alone cannot tie the GPU model to the reference path:
    these logits have a standard deviation of 0.33 and a maximum of 1.4, and
    at rtol=5e-2, atol=5e-1 the model still passed with RoPE removed
    entirely (cos=1, sin=0: max logit difference 0.049) and with the SwiGLU
    output multiplied by 1.3 (max difference 0.24). The logits rule rejects
    both (test_model_float64.py::test_rule_catches_wrong_models)."""
    model, cfg = _tiny_model("cuda")
    cpu_model, _ = _tiny_model("cpu")
    cpu_model.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    x = torch.randint(0, cfg.vocab_size, (2, 32), device="cuda")
    with torch.no_grad():
        lg = model(x).float().cpu()
        lc = cpu_model(x.cpu()).float()
    torch.testing.assert_close(lg, lc, rtol=5e-2, atol=5e-1)
    ref64, base = logits_references(model.state_dict(), cfg, x)
    assert_logits_rule("tiny/forward", lg, ref64, base)


def test_generate_kv_cache_matches_recompute():
    """Greedy decode through the KV cache must produce the same tokens as
    naive full-recompute argmax at every step (fp32 CPU)."""
    torch.manual_seed(7)
    cfg = llama_tiny()
    model = Llama(cfg).eval()
    B, S0, new = 2, 9, 8
    prompt = torch.randint(0, cfg.vocab_size, (B, S0))

    out = model.generate(prompt, max_new_tokens=new)
    assert out.shape == (B, S0 + new)
    assert (out[:, :S0] == prompt).all()

    # naive reference: re-run the full forward for each next token
    toks = prompt.clone()
    with torch.no_grad():
        for _ in range(new):
            nxt = model(toks)[:, -1].argmax(-1, keepdim=True)
            toks = torch.cat([toks, nxt], dim=1)
    assert (out == toks).all(), (out, toks)


def test_generate_sampling_and_stop():
    torch.manual_seed(8)
    cfg = llama_tiny()
    model = Llama(cfg).eval()
    prompt = torch.randint(0, cfg.vocab_size, (1, 5))
    torch.manual_seed(0)
    out = model.generate(prompt, max_new_tokens=6, temperature=0.8, top_k=10)
    assert out.shape[1] <= 11 and out.shape[1] > 5
    # stop token: force it by asking for the greedy first token as stop
    first = model.generate(prompt, max_new_tokens=1)[:, -1].item()
    out2 = model.generate(prompt, max_new_tokens=6, stop_token=first)
    assert out2.shape[1] == 6  # stopped right after the first new token


@pytest.mark.gpu
def test_generate_gpu_cache_logits_match():
    """bf16 GPU decode: per-step cached logits vs full-recompute logits.
    (argmax equality is not robust in bf16, so compare the logits.)

    Cached and recomputed logits are also held to the float64 reference of
    test_model_float64.py under its logits rule. The assert_close alone
    compares the GPU model with itself, and at rtol=5e-2, atol=5e-1 on
    logits of standard deviation 0.33 even the comparison with the CPU path
    passed with RoPE removed (max logit difference 0.049) and with the
    SwiGLU output multiplied by 1.3 (max difference 0.24); the logits rule
    rejects both (test_model_float64.py::test_rule_catches_wrong_models)."""
    model, cfg = _tiny_model("cuda")
    model.eval()
    B, S0 = 2, 7
    prompt = torch.randint(0, cfg.vocab_size, (B, S0), device="cuda")
    from kubetorch_amd.models import KVCache

    cache = KVCache(cfg, B, 32, torch.device("cuda"), torch.bfloat16)
    with torch.no_grad():
        lg_cache = model._forward_cached(prompt, cache)
        lg_full = model(prompt)[:, -1]
        torch.testing.assert_close(lg_cache.float(), lg_full.float(),
                                   rtol=5e-2, atol=5e-1)
        nxt = lg_full.argmax(-1, keepdim=True)
        lg_cache2 = model._forward_cached(nxt, cache)
        toks = torch.cat([prompt, nxt], dim=1)
        lg_full2 = model(toks)[:, -1]
        torch.testing.assert_close(lg_cache2.float(), lg_full2.float(),
                                   rtol=5e-2, atol=5e-1)
        ref64, base = logits_references(model.state_dict(), cfg, toks)
        rows = torch.arange(B)
        for tag, got, pos in (("prefill", lg_cache, S0 - 1),
                              ("prefill_full", lg_full, S0 - 1),
                              ("step", lg_cache2, S0),
                              ("step_full", lg_full2, S0)):
            assert_logits_rule(f"tiny/cache_{tag}", got, ref64, base,
                               rows=(rows, torch.full((B,), pos)))
    out = model.generate(prompt, max_new_tokens=4)
    assert out.shape == (B, S0 + 4) and out.is_cuda


def test_gradient_checkpointing_grads_match():
    """Per-layer checkpointing must reproduce the exact grads of the
    standard forward (fp32 CPU: bit-identical recompute)."""
    torch.manual_seed(11)
    cfg = llama_tiny()
    m1 = Llama(cfg)
    m2 = Llama(cfg)
    m2.load_state_dict(m1.state_dict())
    m2.gradient_checkpointing_enable()
    x = torch.randint(0, cfg.vocab_size, (2, 32))
    y = torch.randint(0, cfg.vocab_size, (2, 32))
    m1.loss(x, y).backward()
    m2.loss(x, y).backward()
    for (n, p1), p2 in zip(m1.named_parameters(), m2.parameters()):
        assert p2.grad is not None, n
        torch.testing.assert_close(p1.grad, p2.grad, rtol=1e-5, atol=1e-6,
                                   msg=n)


def test_hf_checkpoint_roundtrip(tmp_path):
    """kt -> HF safetensors export -> load_hf_checkpoint must reproduce
    the exact model (fused wqkv/gate_up split + concat are inverses)."""
    import json

    from safetensors.torch import save_file

    from kubetorch_amd.models import convert

    torch.manual_seed(21)
    cfg = llama_tiny()
    src = Llama(cfg)
    hf_sd = convert.kt_to_hf_state_dict(src.state_dict(), cfg)
    # HF checkpoints shard weights; emulate two shards
    keys = sorted(hf_sd)
    half = len(keys) // 2
    save_file({k: hf_sd[k].contiguous() for k in keys[:half]},
              str(tmp_path / "model-00001-of-00002.safetensors"))
    save_file({k: hf_sd[k].contiguous() for k in keys[half:]},
              str(tmp_path / "model-00002-of-00002.safetensors"))
    (tmp_path / "config.json").write_text(json.dumps({
        "hidden_size": cfg.dim, "num_hidden_layers": cfg.n_layers,
        "num_attention_heads": cfg.n_heads,
        "num_key_value_heads": cfg.n_kv_heads,
        "intermediate_size": cfg.intermediate,
        "vocab_size": cfg.vocab_size, "max_position_embeddings": cfg.max_seq_len,
        "rope_theta": cfg.rope_base, "rms_norm_eps": cfg.norm_eps,
    }))

    model = convert.load_hf_checkpoint(str(tmp_path), dtype=torch.float32)
    assert model.cfg.dim == cfg.dim and model.cfg.n_kv_heads == cfg.n_kv_heads
    x = torch.randint(0, cfg.vocab_size, (2, 16))
    with torch.no_grad():
        torch.testing.assert_close(model(x), src(x), rtol=1e-5, atol=1e-5)
    # tied-embeddings fallback: drop lm_head from the HF dict
    hf_sd2 = dict(hf_sd)
    hf_sd2.pop("lm_head.weight")
    kt_sd = convert.hf_to_kt_state_dict(hf_sd2, cfg)
    torch.testing.assert_close(kt_sd["lm_head.weight"],
                               hf_sd["model.embed_tokens.weight"])


def test_tokenizer_hf_roundtrip(tmp_path):
    """Train a tiny in-test BPE (offline) and round-trip through the
    serving tokenizer wrapper."""
    from tokenizers import Tokenizer as HFTok
    from tokenizers.models import BPE
    from tokenizers.pre_tokenizers import Whitespace
    from tokenizers.trainers import BpeTrainer

    tok = HFTok(BPE(unk_token="[UNK]"))
    tok.pre_tokenizer = Whitespace()
    tok.train_from_iterator(
        ["the quick brown fox", "jumps over the lazy dog",
         "pack my box with five dozen liquor jugs"] * 20,
        BpeTrainer(vocab_size=200, special_tokens=["[UNK]", "<s>", "</s>"]))
    tok.save(str(tmp_path / "tokenizer.json"))

    from kubetorch_amd.models.tokenizer import Tokenizer

    t = Tokenizer.load(str(tmp_path))  # resolves the file inside the dir
    ids = t.encode("the quick brown fox")
    assert ids and all(isinstance(i, int) for i in ids)
    assert "quick" in t.decode(ids)
    assert t.vocab_size > 0


def test_batched_generator_matches_generate():
    """Continuous batching: requests of different lengths arriving together
    must each produce the same greedy tokens as a solo model.generate."""
    from kubetorch_amd.models.serving import BatchedGenerator

    torch.manual_seed(31)
    cfg = llama_tiny()
    model = Llama(cfg).eval()
    prompts = [[1, 2, 3], [7, 8, 9, 10, 11], [42]]
    new = [6, 4, 5]

    refs = []
    for p, n in zip(prompts, new):
        refs.append(model.generate(torch.tensor([p]), n)[0].tolist())

    eng = BatchedGenerator(model, max_batch=4, max_len=64)
    rids = [eng.submit(p, max_new_tokens=n) for p, n in zip(prompts, new)]
    out = eng.run()
    assert set(out) == set(rids)
    for rid, ref in zip(rids, refs):
        assert out[rid] == ref, (rid, out[rid], ref)


def test_batched_generator_continuous_admission():
    """A request submitted while others are mid-decode joins a free slot
    and still matches its solo output; stop_token exits early."""
    from kubetorch_amd.models.serving import BatchedGenerator

    torch.manual_seed(33)
    cfg = llama_tiny()
    model = Llama(cfg).eval()
    eng = BatchedGenerator(model, max_batch=2, max_len=64)

    r1 = eng.submit([5, 6, 7], max_new_tokens=8)
    r2 = eng.submit([9, 10], max_new_tokens=8)
    eng.step()
    eng.step()
    r3 = eng.submit([20, 21, 22, 23], max_new_tokens=3)  # waits for a slot
    while eng.has_work:
        eng.step()
    out = {**eng.finished}

    for rid, p, n in ((r1, [5, 6, 7], 8), (r2, [9, 10], 8),
                      (r3, [20, 21, 22, 23], 3)):
        ref = model.generate(torch.tensor([p]), n)[0].tolist()
        assert out[rid] == ref, (rid, out[rid], ref)

    # stop token: solo generate stops right after emitting it
    first = model.generate(torch.tensor([[5, 6, 7]]), 1)[0, -1].item()
    eng2 = BatchedGenerator(model, max_batch=1, max_len=32)
    rid = eng2.submit([5, 6, 7], max_new_tokens=8, stop_token=first)
    out2 = eng2.run()
    assert out2[rid][-1] == first and len(out2[rid]) == 4


def test_tokenizer_sentencepiece_roundtrip(tmp_path):
    import sentencepiece as spm

    corpus = tmp_path / "corpus.txt"
    corpus.write_text("\n".join(
        ["the quick brown fox jumps over the lazy dog",
         "pack my box with five dozen liquor jugs"] * 30))
    spm.SentencePieceTrainer.Train(
        input=str(corpus), model_prefix=str(tmp_path / "tokenizer"),
        vocab_size=80, model_type="bpe")

    from kubetorch_amd.models.tokenizer import Tokenizer

    t = Tokenizer.load(str(tmp_path / "tokenizer.model"))
    assert t.kind == "sp"
    ids = t.encode("the quick brown fox", add_bos=True)
    assert ids[0] == t.bos_id
    assert "quick" in t.decode(ids)


def test_chunked_prefill_matches_full():
    """Prefilling the prompt in 3-token chunks must produce the same greedy
    output as the single-chunk prefill (offset-causal mask path)."""
    torch.manual_seed(41)
    cfg = llama_tiny()
    model = Llama(cfg).eval()
    prompt = torch.randint(0, cfg.vocab_size, (2, 10))
    full = model.generate(prompt, max_new_tokens=6)
    chunked = model.generate(prompt, max_new_tokens=6, prefill_chunk=3)
    assert (full == chunked).all(), (full, chunked)


def test_batched_generator_chunked_prefill():
    from kubetorch_amd.models.serving import BatchedGenerator

    torch.manual_seed(43)
    cfg = llama_tiny()
    model = Llama(cfg).eval()
    eng = BatchedGenerator(model, max_batch=2, max_len=64, prefill_chunk=4)
    rid = eng.submit(list(range(1, 11)), max_new_tokens=5)
    out = eng.run()
    ref = model.generate(torch.tensor([list(range(1, 11))]), 5)[0].tolist()
    assert out[rid] == ref


def test_kv_cache_overflow_and_submit_validation():
    from kubetorch_amd.models import KVCache
    from kubetorch_amd.models.serving import BatchedGenerator

    cfg = llama_tiny()
    cache = KVCache(cfg, 1, 8, torch.device("cpu"), torch.float32)
    model = Llama(cfg)
    model._forward_cached(torch.randint(0, cfg.vocab_size, (1, 8)), cache)
    with pytest.raises(RuntimeError, match="overflow"):
        model._forward_cached(torch.randint(0, cfg.vocab_size, (1, 1)), cache)

    eng = BatchedGenerator(model, max_batch=1, max_len=16)
    with pytest.raises(ValueError, match="exceeds"):
        eng.submit(list(range(10)), max_new_tokens=10)


def test_hf_convert_rejects_mismatched_dict(tmp_path):
    import json

    from safetensors.torch import save_file

    from kubetorch_amd.models import convert

    cfg = llama_tiny()
    src = Llama(cfg)
    hf_sd = convert.kt_to_hf_state_dict(src.state_dict(), cfg)
    bad = {k: v for k, v in hf_sd.items()
           if "layers.1" not in k}  # drop a whole layer
    save_file({k: v.contiguous() for k, v in bad.items()},
              str(tmp_path / "model.safetensors"))
    (tmp_path / "config.json").write_text(json.dumps({
        "hidden_size": cfg.dim, "num_hidden_layers": cfg.n_layers,
        "num_attention_heads": cfg.n_heads,
        "num_key_value_heads": cfg.n_kv_heads,
        "intermediate_size": cfg.intermediate,
        "vocab_size": cfg.vocab_size}))
    with pytest.raises(KeyError):
        convert.load_hf_checkpoint(str(tmp_path), dtype=torch.float32)


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_decode_graph_matches_eager_gpu():
    """hipGraph-captured decode emits the same greedy tokens as the eager
    path (tiny llama on cuda, continuous batching with staggered joins)."""
    import torch

    from kubetorch_amd.models import BatchedGenerator, Llama, llama_tiny

    cfg = llama_tiny(max_seq_len=192)
    torch.manual_seed(11)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with torch.device("cuda"):
            model = Llama(cfg).eval()
    finally:
        torch.set_default_dtype(prev)
    prompts = [torch.randint(0, cfg.vocab_size, (n,)).tolist()
               for n in (17, 5, 29, 11)]

    def run(graph):
        eng = BatchedGenerator(model, max_batch=3, max_len=96, graph=graph)
        rids = [eng.submit(p, max_new_tokens=12) for p in prompts[:2]]
        # staggered join: 2 more requests arrive after a few steps
        for _ in range(3):
            eng.step()
        rids += [eng.submit(p, max_new_tokens=12) for p in prompts[2:]]
        out = eng.run()
        return [out[r] for r in rids]

    eager = run(False)
    graphed = run(True)
    assert eager == graphed
