"""Paged prefill and the prefix cache: PagedKVCache(prefix_cache=True) and
BatchedGenerator(kv="paged", prefill="paged", prefix_cache=True).

Allocator tests are host logic on the CPU. Engine tests follow
tests/test_paged_engine.py: on the CPU fp32 tiny llamas and exact greedy
equality with a solo model.generate; on the GPU bf16, graph against eager
exactly and every emitted token against the uncached forward's logits
(_assert_teacher_forced and its tolerance are copied from that file).
"""
import random

import pytest
import torch

from kubetorch_amd.models import (BatchedGenerator, Llama, PagedKVCache,
                                  llama_tiny)

PS = 16


# ---------------------------------------------------------------------------
# Allocator
# ---------------------------------------------------------------------------
def _cache(num_pages=10, page_size=PS, max_batch=4, max_blocks=6,
           prefix_cache=True):
    return PagedKVCache(llama_tiny(), num_pages, page_size, max_batch,
                        max_blocks, torch.device("cpu"), torch.float32,
                        prefix_cache=prefix_cache)


def _trie_nodes(c):
    nodes, stack = [], list(c._root.children.values())
    while stack:
        n = stack.pop()
        nodes.append(n)
        stack.extend(n.children.values())
    return nodes


def _check_invariants(c):
    listed = [0] * c.num_pages
    for slot in range(c.max_batch):
        pages = c.pages_of(slot)
        row = c.block_table[slot].tolist()
        assert row[:len(pages)] == pages
        assert all(p == -1 for p in row[len(pages):])
        assert len(pages) == len(set(pages))
        for p in pages:
            listed[p] += 1
    # a page's refcount is the number of slots listing it
    assert listed == c._ref
    free, idle = list(c._free), list(c._idle)
    assert len(set(free)) == len(free) and not set(free) & set(idle)
    for p in range(c.num_pages):
        held = c._ref[p] > 0
        # held, free and idle partition the pool
        assert held + (p in free) + (p in idle) == 1, p
    assert c.free_pages == len(free) + len(idle)
    # trie nodes and registered pages are in bijection
    nodes = _trie_nodes(c)
    assert sorted(n.page for n in nodes) == sorted(c._node_of)
    assert len(nodes) == len(set(n.page for n in nodes))
    for n in nodes:
        assert c._node_of[n.page] is n
        assert n.parent.children[n.key] is n and len(n.key) == c.page_size
        if n.parent is not c._root:
            assert c._ref[n.parent.page] >= c._ref[n.page]
    assert set(idle) <= set(c._node_of)
    assert not set(free) & set(c._node_of)


def _snapshot(c):
    return (list(c._ref), c.block_table.clone(), list(c._free),
            list(c._idle), sorted(c._node_of),
            [c.pages_of(s) for s in range(c.max_batch)])


def _same(a, b):
    return all(torch.equal(x, y) if torch.is_tensor(x) else x == y
               for x, y in zip(a, b))


def test_prefix_cache_off_is_the_plain_allocator():
    c = _cache(prefix_cache=False)
    assert c.reserve(0, 17) and c.reserve(1, 16)
    assert c.free_pages == 7 and c.pages_of(0) == [0, 1]
    with pytest.raises(RuntimeError):
        c.reserve_prefix(2, list(range(20)), 24)
    with pytest.raises(RuntimeError):
        c.publish(0, list(range(17)))
    c.release(0)
    assert c.reserve(2, 1) and c.pages_of(2) == [0]  # LIFO, as before


def test_prefix_cache_random_operations():
    rng = random.Random(7)
    c = _cache(num_pages=12, max_batch=5, max_blocks=5)
    bases = [[rng.randrange(50) for _ in range(70)] for _ in range(3)]
    live, published = {}, set()
    hits = 0
    for _ in range(400):
        slot = rng.randrange(c.max_batch)
        if slot not in live:
            base = rng.choice(bases)
            prompt = base[:rng.randint(1, 60)]
            if rng.random() < 0.5:
                prompt = prompt + [rng.randrange(50, 60)
                                   for _ in range(rng.randint(0, 8))]
            n = min(len(prompt) + rng.randint(1, 12), 5 * PS)
            prompt = prompt[:n - 1]
            before = _snapshot(c)
            free = c.free_pages
            got = c.reserve_prefix(slot, prompt, n)
            if got is None:
                assert _same(before, _snapshot(c))
                assert -(-n // PS) > free  # never fails with room
            else:
                assert got % PS == 0 and got <= (len(prompt) - 1) // PS * PS
                hits += got
                live[slot] = prompt
        elif slot not in published and rng.random() < 0.6:
            c.publish(slot, live[slot])
            published.add(slot)
        else:
            c.release(slot)
            del live[slot]
            published.discard(slot)
        _check_invariants(c)
    assert hits > 0 and c.evicted_pages > 0
    for slot in list(live):
        c.release(slot)
    _check_invariants(c)
    assert c.free_pages == c.num_pages


def test_prefix_match_is_capped_below_the_whole_prompt():
    """At least one prompt token is computed: a 32-token prompt resubmitted
    with 16-token pages hits 16 tokens, not 32."""
    c = _cache()
    prompt = list(range(32))
    assert c.reserve_prefix(0, prompt, 40) == 0
    c.publish(0, prompt)
    assert len(c._node_of) == 2
    assert c.reserve_prefix(1, prompt, 40) == 16
    assert c.pages_of(1)[0] == c.pages_of(0)[0]
    assert c.pages_of(1)[1] != c.pages_of(0)[1]
    assert c.reserve_prefix(2, prompt + [99], 40) == 32
    assert c.pages_of(2)[:2] == c.pages_of(0)[:2]
    # the existing node stays registered, the own copy stays private
    own = c.pages_of(1)[1]
    c.publish(1, prompt)
    assert own not in c._node_of and len(c._node_of) == 2
    _check_invariants(c)


def test_failed_reserve_prefix_changes_nothing():
    c = _cache(num_pages=4)
    prompt = list(range(33))
    assert c.reserve_prefix(0, prompt, 40) == 0       # 3 pages
    c.publish(0, prompt)
    c.release(0)                                       # 2 idle, 2 free
    assert c.reserve_prefix(1, list(range(100, 120)), 20) == 0  # 2 free taken
    before = _snapshot(c)
    assert c.free_pages == 2
    # matches both idle pages, needs 1 more: nothing left once they are pinned
    assert c.reserve_prefix(2, prompt, 40) is None
    assert _same(before, _snapshot(c))
    assert c.reserve(3, 3 * PS) is False               # through reserve() too
    assert _same(before, _snapshot(c))
    _check_invariants(c)


def test_pinned_pages_are_not_evicted_for_their_own_request():
    c = _cache(num_pages=5)
    P = list(range(33))
    Q = list(range(200, 217))
    assert c.reserve_prefix(0, P, 40) == 0
    c.publish(0, P)
    a0, a1 = c.pages_of(0)[:2]
    c.release(0)
    assert c.reserve_prefix(0, Q, 17) == 0
    c.publish(0, Q)
    q0 = c.pages_of(0)[0]
    c.release(0)
    # idle, least recently used first: a1, a0, q0. B matches a0 and a1 and
    # needs 3 more pages with 2 free: the one eviction must take q0
    assert list(c._idle) == [a1, a0, q0] and len(c._free) == 2
    B = P[:32] + [77, 78]
    assert c.reserve_prefix(1, B, 5 * PS) == 32
    assert c.pages_of(1)[:2] == [a0, a1]
    assert c.evicted_pages == 1 and q0 not in c._node_of
    assert q0 in c.pages_of(1)
    _check_invariants(c)
    # q0 now holds other content: the old prompt misses
    c.release(1)
    assert c.reserve_prefix(2, Q, 17) == 0
    _check_invariants(c)


def test_evicting_a_node_drops_its_subtree():
    c = _cache(num_pages=4)
    P = list(range(49))
    assert c.reserve_prefix(0, P, 50) == 0            # all 4 pages
    c.publish(0, P)
    a0, a1, a2 = c.pages_of(0)[:3]
    c.release(0)
    assert c.free_pages == 4 and len(c._idle) == 3
    c._idle.move_to_end(a0, last=False)   # make the root-most node the LRU
    assert c.reserve_prefix(1, list(range(300, 320)), 2 * PS) == 0
    # one free page + one eviction, which dropped a0 with a1 and a2
    assert c.evicted_pages == 3
    assert not c._node_of and not c._idle and not c._root.children
    _check_invariants(c)
    c.release(1)
    assert c.reserve_prefix(2, P, 50) == 0            # a full miss
    c.release(2)
    assert c.free_pages == c.num_pages


# ---------------------------------------------------------------------------
# Engine, CPU
# ---------------------------------------------------------------------------
def _solo(model, prompt, n, **kw):
    return model.generate(torch.tensor([prompt]), n, **kw)[0].tolist()


def _model(seed):
    torch.manual_seed(seed)
    return Llama(llama_tiny()).eval()


def test_engine_option_validation():
    model = _model(37)
    for kw in ({"prefill": "paged"}, {"prefix_cache": True},
               {"kv": "slot", "prefill": "paged"}):
        with pytest.raises(ValueError, match="kv='paged'"):
            BatchedGenerator(model, max_batch=2, max_len=64, **kw)
    with pytest.raises(ValueError, match="prefill"):
        BatchedGenerator(model, max_batch=2, max_len=64, kv="paged",
                         prefill="ring")
    eng = BatchedGenerator(model, max_batch=2, max_len=64, kv="paged")
    assert eng._prefill_paged is False and eng._pkv.prefix_cache is False
    eng = BatchedGenerator(model, max_batch=2, max_len=64, kv="paged",
                           prefix_cache=True)
    assert eng._prefill_paged is True and eng._pkv.prefix_cache is True


def test_paged_prefill_allocates_no_kv_cache(monkeypatch):
    import kubetorch_amd.models.llama as llama

    def boom(*a, **k):
        raise AssertionError("prefill='paged' built a KVCache")
    model = _model(31)
    ref = _solo(model, list(range(20, 38)), 4)
    monkeypatch.setattr(llama, "KVCache", boom)
    eng = BatchedGenerator(model, max_batch=2, max_len=64, kv="paged",
                           prefill="paged")
    rid = eng.submit(list(range(20, 38)), max_new_tokens=4)
    assert eng.run()[rid] == ref


def test_paged_prefill_matches_generate():
    """Mixed lengths in one packed forward, two of them crossing a page."""
    model = _model(31)
    prompts = [[1, 2, 3], [7, 8, 9, 10, 11], [42],
               list(range(20, 34)), list(range(40, 56)), list(range(60, 93))]
    new = [6, 4, 5, 6, 3, 4]
    refs = [_solo(model, p, n) for p, n in zip(prompts, new)]
    eng = BatchedGenerator(model, max_batch=6, max_len=64, kv="paged",
                           page_size=16, prefill="paged")
    rids = [eng.submit(p, max_new_tokens=n) for p, n in zip(prompts, new)]
    out = eng.run()
    for rid, ref in zip(rids, refs):
        assert out[rid] == ref, (rid, out[rid], ref)
    assert eng._pkv.free_pages == eng._pkv.num_pages


@pytest.mark.parametrize("page_size", [16, 32])
def test_paged_prefill_chunked(page_size):
    """prefill_chunk=4: packed rounds inside one step(), requests leaving
    the rounds at different times."""
    model = _model(43)
    prompts = [list(range(1, 19)), [3, 4, 5], list(range(30, 63)),
               list(range(70, 78))]
    eng = BatchedGenerator(model, max_batch=4, max_len=64, prefill_chunk=4,
                           kv="paged", page_size=page_size, prefill="paged")
    rids = [eng.submit(p, max_new_tokens=5) for p in prompts]
    eng.step()
    assert all(len(eng.slots[s].out) == len(p) + 2   # prefill + one decode
               for s, p in enumerate(prompts))
    out = eng.run()
    for rid, p in zip(rids, prompts):
        assert out[rid] == _solo(model, p, 5), rid
    assert eng._pkv.free_pages == eng._pkv.num_pages


def test_paged_prefill_small_pool_waits_for_pages():
    model = _model(35)
    reqs = [(list(range(20, 34)), 6),    # 20 tokens -> 2 pages
            (list(range(40, 56)), 3),    # 19 tokens -> 2 pages
            ([5, 6, 7, 8, 9], 4)]        # 9 tokens -> 1 page
    eng = BatchedGenerator(model, max_batch=3, max_len=64, kv="paged",
                           page_size=16, num_pages=4, prefill="paged")
    rids = [eng.submit(p, max_new_tokens=n) for p, n in reqs]
    eng.step()
    assert eng.slots[2] is None and len(eng.pending) == 1
    assert eng._pkv.free_pages == 0
    out = eng.run()
    for rid, (p, n) in zip(rids, reqs):
        assert out[rid] == _solo(model, p, n), rid
    assert eng._pkv.free_pages == eng._pkv.num_pages == 4


def test_paged_prefill_moe_matches_cache_prefill():
    from kubetorch_amd.models.moe import convert_to_moe

    torch.manual_seed(41)
    model = Llama(llama_tiny())
    convert_to_moe(model, n_experts=4, top_k=2)
    model.eval()
    prompts = [[1, 2, 3, 4], list(range(10, 27))]
    outs = []
    for prefill in ("cache", "paged"):
        eng = BatchedGenerator(model, max_batch=2, max_len=64, kv="paged",
                               prefill=prefill)
        rids = [eng.submit(p, max_new_tokens=5) for p in prompts]
        out = eng.run()
        outs.append([out[r] for r in rids])
    assert outs[0] == outs[1]


PREFIX = list(range(100, 140))           # 40 tokens: 2 full pages of 16 + 8


def test_prefix_hit_after_completion():
    model = _model(47)
    A, B = PREFIX + [1, 2, 3], PREFIX + [9, 8]
    eng = BatchedGenerator(model, max_batch=2, max_len=64, kv="paged",
                           page_size=16, prefix_cache=True)
    ra = eng.submit(A, max_new_tokens=5)
    out = eng.run()
    assert out[ra] == _solo(model, A, 5)
    assert eng.cached_tokens[ra] == 0
    assert eng._pkv.free_pages == eng._pkv.num_pages
    assert len(eng._pkv._idle) == 2       # A's full prompt pages stay cached
    rb = eng.submit(B, max_new_tokens=6)
    eng.step()
    assert eng.slots[0].cached_tokens == 32 and eng.cached_tokens[rb] == 32
    out = eng.run()
    assert out[rb] == _solo(model, B, 6)
    assert eng.prefix_stats == {"prompt_tokens": len(A) + len(B),
                                "hit_tokens": 32, "evicted_pages": 0}
    assert eng._pkv.free_pages == eng._pkv.num_pages


def test_prefix_shared_with_a_live_request():
    """B joins while A decodes and shares A's two prompt pages (refcount
    2); A finishes first and B goes on reading them. C, admitted in the
    same step as B, does not see B's pages, only A's."""
    model = _model(49)
    A, B, C = PREFIX + [1, 2, 3], PREFIX + [9, 8], PREFIX + [9, 8, 7, 6, 5]
    eng = BatchedGenerator(model, max_batch=3, max_len=80, kv="paged",
                           page_size=16, prefix_cache=True)
    ra = eng.submit(A, max_new_tokens=6)
    eng.step()
    eng.step()
    rb = eng.submit(B, max_new_tokens=9)
    rc = eng.submit(C, max_new_tokens=3)
    eng.step()
    pkv = eng._pkv
    shared = pkv.pages_of(0)[:2]
    assert pkv.pages_of(1)[:2] == shared and pkv.pages_of(2)[:2] == shared
    assert [pkv._ref[p] for p in shared] == [3, 3]
    assert pkv._ref[pkv.pages_of(1)[2]] == 1
    assert eng.cached_tokens == {ra: 0, rb: 32, rc: 32}
    while ra not in eng.finished:
        eng.step()
    assert eng.slots[1] is not None, "B must outlive A"
    assert rc in eng.finished and [pkv._ref[p] for p in shared] == [1, 1]
    out = eng.run()
    assert out[ra] == _solo(model, A, 6)
    assert out[rb] == _solo(model, B, 9)
    assert out[rc] == _solo(model, C, 3)
    assert eng.prefix_stats == {"prompt_tokens": len(A) + len(B) + len(C),
                                "hit_tokens": 64, "evicted_pages": 0}
    assert pkv.free_pages == pkv.num_pages


def test_prefix_eviction_in_a_small_pool():
    """4 pages: A's idle prefix (2 pages) cannot survive D, which needs all
    4; A's prompt then misses, and everything is still right."""
    model = _model(51)
    A = PREFIX + [1, 2, 3]
    D = list(range(300, 350))
    eng = BatchedGenerator(model, max_batch=2, max_len=64, kv="paged",
                           page_size=16, num_pages=4, prefix_cache=True)
    ra = eng.submit(A, max_new_tokens=5)
    assert eng.run()[ra] == _solo(model, A, 5)
    rd = eng.submit(D, max_new_tokens=6)      # 56 tokens -> 4 pages
    assert eng.run()[rd] == _solo(model, D, 6)
    assert eng.prefix_stats["evicted_pages"] == 2
    ra2 = eng.submit(A, max_new_tokens=5)
    out = eng.run()
    assert out[ra2] == _solo(model, A, 5)
    assert eng.cached_tokens[ra2] == 0
    assert eng.prefix_stats["prompt_tokens"] == 2 * len(A) + len(D)
    assert eng.prefix_stats["hit_tokens"] == 0
    assert eng.prefix_stats["evicted_pages"] > 2   # D's pages went as well
    assert eng._pkv.free_pages == eng._pkv.num_pages == 4


def test_prefix_cache_with_chunked_prefill():
    model = _model(53)
    A, B = PREFIX + [1, 2, 3], PREFIX + list(range(200, 213))
    eng = BatchedGenerator(model, max_batch=2, max_len=80, kv="paged",
                           page_size=16, prefix_cache=True, prefill_chunk=4)
    ra = eng.submit(A, max_new_tokens=3)
    assert eng.run()[ra] == _solo(model, A, 3)
    rb = eng.submit(B, max_new_tokens=4)
    assert eng.run()[rb] == _solo(model, B, 4)
    assert eng.cached_tokens[rb] == 32


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


def _gpu_prompts(cfg, lens=(17, 5, 29, 11)):
    gen = torch.Generator().manual_seed(3)
    return [torch.randint(0, cfg.vocab_size, (n,), generator=gen).tolist()
            for n in lens]


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
def test_paged_prefill_staggered_join_gpu(gpu_model):
    model = gpu_model
    prompts = _gpu_prompts(model.cfg)

    def run(graph):
        eng = BatchedGenerator(model, max_batch=3, max_len=96, graph=graph,
                               kv="paged", page_size=16, prefill="paged")
        rids = [eng.submit(p, max_new_tokens=12) for p in prompts[:2]]
        for _ in range(3):  # staggered join
            eng.step()
        rids += [eng.submit(p, max_new_tokens=12) for p in prompts[2:]]
        out = eng.run()
        assert eng._pkv.free_pages == eng._pkv.num_pages
        return [out[r] for r in rids]

    eager, graphed = run(False), run(True)
    assert eager == graphed
    for p, toks in zip(prompts, graphed):
        assert len(toks) == len(p) + 12
        _assert_teacher_forced(model, len(p), toks)


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_prefix_cache_graph_matches_eager_gpu(gpu_model):
    """A and B (same 40-token prefix) are live together and share two pages
    during the captured decode step; C, a hit as well, is admitted after
    the graph was captured and while A's pages are idle or shared."""
    model = gpu_model
    prefix, ta, tb, tc = _gpu_prompts(model.cfg, (40, 3, 7, 21))
    reqs = [(prefix + ta, 10), (prefix + tb, 16), (prefix + tc, 8)]

    def run(graph):
        eng = BatchedGenerator(model, max_batch=2, max_len=96, graph=graph,
                               kv="paged", page_size=16, prefix_cache=True)
        ra = eng.submit(reqs[0][0], max_new_tokens=reqs[0][1])
        eng.step()
        eng.step()
        rb = eng.submit(reqs[1][0], max_new_tokens=reqs[1][1])
        eng.step()
        pkv = eng._pkv
        shared = pkv.pages_of(0)[:2]
        assert pkv.pages_of(1)[:2] == shared
        assert [pkv._ref[p] for p in shared] == [2, 2]
        if graph:
            assert len(eng._graphs) == 1
        rc = eng.submit(reqs[2][0], max_new_tokens=reqs[2][1])  # waits
        out = eng.run()
        assert eng.cached_tokens == {ra: 0, rb: 32, rc: 32}
        assert eng.prefix_stats["hit_tokens"] == 64
        assert pkv.free_pages == pkv.num_pages
        return [out[r] for r in (ra, rb, rc)]

    eager, graphed = run(False), run(True)
    assert eager == graphed
    for (p, n), toks in zip(reqs, graphed):
        assert len(toks) == len(p) + n
        _assert_teacher_forced(model, len(p), toks)
