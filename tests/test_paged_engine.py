"""Paged KV cache in the serving engine: the PagedKVCache allocator and
BatchedGenerator(kv="paged").

CPU tests run fp32 tiny llamas and require exact greedy-token equality
with a solo model.generate, as the slot-cache engine tests do. GPU tests
run bf16, where argmax equality against an independent computation is not
robust; they compare graph with eager exactly (same kernels, deterministic)
and check every emitted token against the uncached forward's logits.
"""
import random

import pytest
import torch

from kubetorch_amd.models import (BatchedGenerator, Llama, PagedKVCache,
                                  llama_tiny)


# ---------------------------------------------------------------------------
# Allocator (host logic; CPU only)
# ---------------------------------------------------------------------------
def _cache(num_pages=10, page_size=16, max_batch=4, max_blocks=6):
    return PagedKVCache(llama_tiny(), num_pages, page_size, max_batch,
                        max_blocks, torch.device("cpu"), torch.float32)


def _check_invariants(c, live):
    """live: slot -> reserved token count."""
    seen = []
    for slot in range(c.max_batch):
        pages = c.pages_of(slot)
        row = c.block_table[slot].tolist()
        if slot in live:
            assert len(pages) == -(-live[slot] // c.page_size)
        else:
            assert pages == []
        assert row[:len(pages)] == pages
        assert all(p == -1 for p in row[len(pages):])
        assert all(0 <= p < c.num_pages for p in pages)
        seen += pages
    assert len(seen) == len(set(seen)), "a page is owned twice"
    assert c.free_pages == c.num_pages - len(seen)


def test_paged_cache_reserve_release_accounting():
    c = _cache()
    assert c.free_pages == 10
    assert c.block_table.dtype == torch.int32
    assert c.block_table.shape == (4, 6) and bool((c.block_table == -1).all())
    assert c.k[0].shape == (10, 2, 16, 64) and len(c.k) == len(c.v) == 2
    assert c.reserve(0, 17) is True       # 2 pages
    assert c.reserve(2, 16) is True       # 1 page
    assert c.reserve(3, 1) is True        # 1 page
    assert c.free_pages == 6
    _check_invariants(c, {0: 17, 2: 16, 3: 1})
    c.release(2)
    assert bool((c.block_table[2] == -1).all())
    _check_invariants(c, {0: 17, 3: 1})
    c.release(0)
    c.release(3)
    assert c.free_pages == c.num_pages
    _check_invariants(c, {})


def test_paged_cache_short_pool_and_errors():
    c = _cache(num_pages=3)
    assert c.reserve(0, 32) is True
    before = c.block_table.clone()
    assert c.reserve(1, 33) is False      # needs 3, 1 free
    assert c.free_pages == 1 and c.pages_of(1) == []
    assert torch.equal(c.block_table, before)
    assert c.reserve(1, 16) is True
    with pytest.raises(RuntimeError, match="already"):
        c.reserve(0, 1)
    with pytest.raises(RuntimeError, match="no pages"):
        c.release(2)
    with pytest.raises(ValueError):
        c.reserve(2, 6 * 16 + 1)          # more blocks than a row holds
    _check_invariants(c, {0: 32, 1: 16})


def test_paged_cache_random_operations():
    rng = random.Random(5)
    c = _cache(num_pages=12, max_batch=5, max_blocks=4)
    live = {}
    for _ in range(200):
        slot = rng.randrange(c.max_batch)
        if slot in live:
            c.release(slot)
            del live[slot]
        else:
            n = rng.randint(1, 4 * 16)
            free = c.free_pages
            ok = c.reserve(slot, n)
            assert ok == (-(-n // 16) <= free)
            if ok:
                live[slot] = n
        _check_invariants(c, live)
    for slot in list(live):
        c.release(slot)
    assert c.free_pages == c.num_pages


# ---------------------------------------------------------------------------
# Engine, CPU
# ---------------------------------------------------------------------------
def _solo(model, prompt, n, **kw):
    return model.generate(torch.tensor([prompt]), n, **kw)[0].tolist()


def _model(seed):
    torch.manual_seed(seed)
    return Llama(llama_tiny()).eval()


def test_paged_generator_matches_generate():
    """Mixed lengths arriving together, including a prompt of 14 with 6
    new tokens and a prompt of 16 with 3 (both cross a 16-token page)."""
    model = _model(31)
    prompts = [[1, 2, 3], [7, 8, 9, 10, 11], [42],
               list(range(20, 34)), list(range(40, 56))]
    new = [6, 4, 5, 6, 3]
    refs = [_solo(model, p, n) for p, n in zip(prompts, new)]
    eng = BatchedGenerator(model, max_batch=5, max_len=64, kv="paged",
                           page_size=16)
    rids = [eng.submit(p, max_new_tokens=n) for p, n in zip(prompts, new)]
    out = eng.run()
    assert set(out) == set(rids)
    for rid, ref in zip(rids, refs):
        assert out[rid] == ref, (rid, out[rid], ref)
    assert eng._pkv.free_pages == eng._pkv.num_pages


def test_paged_generator_continuous_admission():
    model = _model(33)
    eng = BatchedGenerator(model, max_batch=2, max_len=64, kv="paged")
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
        assert out[rid] == _solo(model, p, n), rid
    first = _solo(model, [5, 6, 7], 1)[-1]
    eng2 = BatchedGenerator(model, max_batch=1, max_len=32, kv="paged")
    rid = eng2.submit([5, 6, 7], max_new_tokens=8, stop_token=first)
    out2 = eng2.run()
    assert out2[rid][-1] == first and len(out2[rid]) == 4
    assert eng2._pkv.free_pages == eng2._pkv.num_pages


@pytest.mark.parametrize("page_size", [16, 32])
def test_paged_generator_prefill_variants(page_size):
    """Chunked prefill (one request) and batched same-length prefill."""
    model = _model(43)
    long = list(range(1, 19))  # 18 tokens: crosses a 16-token page
    eng = BatchedGenerator(model, max_batch=2, max_len=64, prefill_chunk=4,
                           kv="paged", page_size=page_size)
    rid = eng.submit(long, max_new_tokens=5)
    assert eng.run()[rid] == _solo(model, long, 5)

    same = [list(range(30, 47)), list(range(60, 77)), [3, 4, 5]]
    eng = BatchedGenerator(model, max_batch=3, max_len=64, kv="paged",
                           page_size=page_size)
    rids = [eng.submit(p, max_new_tokens=4) for p in same]
    out = eng.run()
    for rid, p in zip(rids, same):
        assert out[rid] == _solo(model, p, 4), rid


def test_paged_generator_small_pool_waits_for_pages():
    """Pages for two of three requests: the third waits although a slot is
    free, is admitted after a finish, and nothing leaks."""
    model = _model(35)
    reqs = [(list(range(20, 34)), 6),    # 20 tokens -> 2 pages
            (list(range(40, 56)), 3),    # 19 tokens -> 2 pages
            ([5, 6, 7, 8, 9], 4)]        # 9 tokens -> 1 page
    eng = BatchedGenerator(model, max_batch=3, max_len=64, kv="paged",
                           page_size=16, num_pages=4)
    rids = [eng.submit(p, max_new_tokens=n) for p, n in reqs]
    eng.step()
    assert eng.slots[2] is None, "a slot must be free"
    assert len(eng.pending) == 1 and eng.pending[0].rid == rids[2]
    assert eng._pkv.free_pages == 0
    waited = 0
    while eng.pending:
        eng.step()
        waited += 1
    assert waited >= 1 and rids[1] in eng.finished  # admitted after a finish
    out = eng.run()
    for rid, (p, n) in zip(rids, reqs):
        assert out[rid] == _solo(model, p, n), rid
    assert eng._pkv.free_pages == eng._pkv.num_pages == 4


def test_paged_generator_submit_and_argument_validation():
    model = _model(37)
    eng = BatchedGenerator(model, max_batch=2, max_len=64, kv="paged",
                           page_size=16, num_pages=2)
    with pytest.raises(ValueError, match="pages"):
        eng.submit(list(range(30)), max_new_tokens=10)   # 3 pages > pool
    with pytest.raises(ValueError, match="exceeds"):
        eng.submit(list(range(60)), max_new_tokens=10)
    eng.submit(list(range(30)), max_new_tokens=2)        # 2 pages fit
    with pytest.raises(ValueError, match="kv"):
        BatchedGenerator(model, max_batch=2, max_len=64, kv="ring")
    # default pool: the slot cache's capacity
    full = BatchedGenerator(model, max_batch=3, max_len=40, kv="paged")
    assert full._pkv.num_pages == 3 * 3 and full._pkv.max_blocks == 3
    assert not hasattr(full, "k")  # no slot slabs next to the pools


def test_slot_mode_explicit_is_default():
    model = _model(39)
    prompts = [[1, 2, 3], [7, 8, 9, 10, 11], [42]]
    outs = []
    for kw in ({}, {"kv": "slot"}):
        eng = BatchedGenerator(model, max_batch=2, max_len=64, **kw)
        assert eng._paged is False and eng.k[0].shape == (2, 2, 64, 64)
        rids = [eng.submit(p, max_new_tokens=5) for p in prompts]
        out = eng.run()
        outs.append([out[r] for r in rids])
    assert outs[0] == outs[1]


def test_paged_generator_moe_matches_slot():
    from kubetorch_amd.models.moe import convert_to_moe

    torch.manual_seed(41)
    model = Llama(llama_tiny())
    convert_to_moe(model, n_experts=4, top_k=2)
    model.eval()
    prompts = [[1, 2, 3, 4], list(range(10, 27))]
    outs = []
    for kv in ("slot", "paged"):
        eng = BatchedGenerator(model, max_batch=2, max_len=64, kv=kv,
                               graph=True)
        assert eng._use_graph is False  # MoE: always eager
        rids = [eng.submit(p, max_new_tokens=5) for p in prompts]
        out = eng.run()
        outs.append([out[r] for r in rids])
    assert outs[0] == outs[1]


# ---------------------------------------------------------------------------
# Engine, GPU (bf16)
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_model():
    cfg = llama_tiny(max_seq_len=192)
    torch.manual_seed(11)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with torch.device("cuda"):
            model = Llama(cfg).eval()
    finally:
        torch.set_default_dtype(prev)
    return model


def _gpu_prompts(cfg):
    gen = torch.Generator().manual_seed(3)
    return [torch.randint(0, cfg.vocab_size, (n,), generator=gen).tolist()
            for n in (17, 5, 29, 11)]


def _assert_teacher_forced(model, prompt_len, tokens):
    """Every emitted token must be within twice the project's cached-vs-
    recompute logits tolerance (0.5 + 0.05*|logit|) of the uncached
    forward's best logit at that position; two independently rounded bf16
    logits are compared, so exact argmax is not required. No position is
    exempt."""
    with torch.no_grad():
        x = torch.tensor([tokens[:-1]], device="cuda")
        logits = model(x)[0].float()
    checked = 0
    for i in range(prompt_len, len(tokens)):
        row = logits[i - 1]
        top = float(row.max())
        got = float(row[tokens[i]])
        assert got >= top - 2 * (0.5 + 0.05 * abs(top)), \
            (i, tokens[i], got, top)
        checked += 1
    assert checked == len(tokens) - prompt_len > 0


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_paged_decode_graph_matches_eager_gpu(gpu_model):
    model = gpu_model
    prompts = _gpu_prompts(model.cfg)

    def run(graph):
        eng = BatchedGenerator(model, max_batch=3, max_len=96, graph=graph,
                               kv="paged", page_size=16)
        rids = [eng.submit(p, max_new_tokens=12) for p in prompts[:2]]
        for _ in range(3):  # staggered join
            eng.step()
        rids += [eng.submit(p, max_new_tokens=12) for p in prompts[2:]]
        out = eng.run()
        assert eng._pkv.free_pages == eng._pkv.num_pages
        return eng, [out[r] for r in rids]

    _, eager = run(False)
    eng, graphed = run(True)
    assert eager == graphed
    assert eng._use_graph and len(eng._graphs) == 1
    for p, toks in zip(prompts, graphed):
        assert len(toks) == len(p) + 12
        _assert_teacher_forced(model, len(p), toks)


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("graph,num_splits", [(False, None), (True, None),
                                              (True, 2)],
                         ids=["eager", "graph", "graph-2splits"])
def test_paged_slot_reuse_reads_no_stale_pages_gpu(gpu_model, graph,
                                                   num_splits):
    """max_batch=2, three requests: the third takes over a freed slot and
    the pages of its previous tenant. At this size the engine picks one
    split; the last case forces two, so the partial buffers and the merge
    kernel are captured too."""
    model = gpu_model
    prompts = _gpu_prompts(model.cfg)[:3]
    eng = BatchedGenerator(model, max_batch=2, max_len=96, graph=graph,
                           kv="paged", page_size=16, num_pages=6,
                           num_splits=num_splits)
    assert eng._num_splits == (num_splits or 1)
    new = [6, 14, 10]
    rids = [eng.submit(p, max_new_tokens=n) for p, n in zip(prompts, new)]
    out = eng.run()
    assert eng._pkv.free_pages == 6
    for rid, p, n in zip(rids, prompts, new):
        assert len(out[rid]) == len(p) + n
        _assert_teacher_forced(model, len(p), out[rid])
