"""Block-table paged KV cache for the serving engine.

Each layer holds one pool of fixed-size pages, [num_pages, n_kv, page_size,
head_dim] for K and for V, instead of a [max_batch, n_kv, max_len, hd] slab
per slot. A sequence owns ceil(tokens/page_size) pages, listed in its row of
the block table; memory and decode reads follow the sequence's own length.

The allocator is host-side and whole-request: BatchedGenerator reserves the
pages for prompt + max_new_tokens at admission, so a row of the table never
changes during a request's life, the captured decode step needs no host work
per token, and a running request cannot run out of pages (no preemption or
swap).

prefix_cache=True (opt-in) lets requests whose prompts start with the same
tokens share whole pages. Registered pages hang in a trie whose edge key is
(parent node, the page's page_size token ids): an exact comparison, so no
hash collision can hand out another prompt's KV. Only pages fully covered by
prompt tokens are registered, and they are never written again (prefill
writes positions >= the cached tokens, decode positions >= the prompt
length), so no copy-on-write is needed. Pages are reference-counted; a
holder of a page holds all its ancestors, so ref(parent) >= ref(child) and
an idle (refcount 0) node's whole subtree is idle. Idle registered pages
stay cached on an LRU list until the allocator needs them; evicting a node
drops its whole subtree from the trie, so no unreachable page stays
registered and a page reused for other content cannot be hit through an
old path.

kv_dtype="fp8" (opt-in) allocates the pools as torch.float8_e4m3fn, one
byte per element, with static fp32 scales per layer and kv head: a byte
encodes x / scale (ops.paged_kv_write quantises, the attention ops
dequantise). Pages are bytes to everything above, so none of it changes.
calibrate_kv_scales derives scales from one prompt.
"""
from collections import OrderedDict

import torch


class _Node:
    __slots__ = ("page", "parent", "key", "children")

    def __init__(self, page, parent, key):
        self.page = page
        self.parent = parent
        self.key = key
        self.children = {}


def _host_scales(scales, cfg, name):
    """[n_layers, n_kv] fp32 on the host, positive and finite; None = ones."""
    shape = (cfg.n_layers, cfg.n_kv_heads)
    if scales is None:
        return torch.ones(shape, dtype=torch.float32)
    s = torch.as_tensor(scales).detach().to("cpu", torch.float32)
    if tuple(s.shape) != shape:
        raise ValueError(f"{name} must be [n_layers, n_kv] = {list(shape)}, "
                         f"got {list(s.shape)}")
    if not bool(((s > 0) & s.isfinite()).all()):
        raise ValueError(f"{name} must be positive and finite")
    return s


class PagedKVCache:
    def __init__(self, cfg, num_pages, page_size, max_batch, max_blocks,
                 device, dtype, prefix_cache=False, kv_dtype=None,
                 k_scales=None, v_scales=None):
        if num_pages < 1 or max_blocks < 1 or max_batch < 1:
            raise ValueError("num_pages, max_blocks and max_batch must be >= 1")
        if kv_dtype not in (None, "fp8"):
            raise ValueError(f"kv_dtype must be None or 'fp8', got {kv_dtype!r}")
        if kv_dtype is None and (k_scales is not None or v_scales is not None):
            raise ValueError("k_scales/v_scales need kv_dtype='fp8'")
        self.num_pages = num_pages
        self.page_size = page_size
        self.max_batch = max_batch
        self.max_blocks = max_blocks
        self.kv_dtype = kv_dtype
        # kv_dtype="fp8": one-byte e4m3 pages (the allocator below deals in
        # pages, not bytes, and is the same) and static per-layer [n_kv]
        # fp32 scales on the device, which ops.paged_* take; None otherwise
        self.k_scale = [None] * cfg.n_layers
        self.v_scale = [None] * cfg.n_layers
        if kv_dtype == "fp8":
            dtype = torch.float8_e4m3fn
            ks = _host_scales(k_scales, cfg, "k_scales").to(device)
            vs = _host_scales(v_scales, cfg, "v_scales").to(device)
            self.k_scale = list(ks.unbind(0))
            self.v_scale = list(vs.unbind(0))
        shape = (num_pages, cfg.n_kv_heads, page_size, cfg.head_dim)
        self.k = [torch.zeros(shape, device=device, dtype=dtype)
                  for _ in range(cfg.n_layers)]
        self.v = [torch.zeros(shape, device=device, dtype=dtype)
                  for _ in range(cfg.n_layers)]
        self.block_table = torch.full((max_batch, max_blocks), -1,
                                      dtype=torch.int32, device=device)
        self._host_table = torch.full((max_batch, max_blocks), -1,
                                      dtype=torch.int32)
        self._owned = [[] for _ in range(max_batch)]
        # LIFO free list: a released request's pages are the next handed out
        self._free = list(range(num_pages - 1, -1, -1))
        self.prefix_cache = bool(prefix_cache)
        self._ref = [0] * num_pages       # slots listing the page
        self._root = _Node(-1, None, None)
        self._node_of = {}                # registered page -> trie node
        self._idle = OrderedDict()        # registered, refcount 0; LRU first
        self.evicted_pages = 0

    @property
    def free_pages(self):
        """Pages an admission can get: free ones plus idle cached ones."""
        return len(self._free) + len(self._idle)

    def pages_of(self, slot):
        return list(self._owned[slot])

    def token_slots(self, slot, start, stop):
        """Physical token indices (page * page_size + offset) of positions
        [start, stop) of `slot`: the slot map paged_kv_write takes."""
        ps, pages = self.page_size, self._owned[slot]
        return [pages[t // ps] * ps + t % ps for t in range(start, stop)]

    def pages_needed(self, n_tokens):
        return -(-n_tokens // self.page_size)

    def reserve(self, slot, n_tokens):
        """Give `slot` the pages for n_tokens tokens and fill its table row.
        Returns False, changing nothing, when not enough pages are free."""
        if self.prefix_cache:
            return self.reserve_prefix(slot, (), n_tokens) is not None
        need = self._check_reserve(slot, n_tokens)
        if need > len(self._free):
            return False
        self._set_row(slot, [self._free.pop() for _ in range(need)])
        return True

    def _check_reserve(self, slot, n_tokens):
        if self._owned[slot]:
            raise RuntimeError(f"slot {slot} already holds pages")
        need = self.pages_needed(n_tokens)
        if need < 1 or need > self.max_blocks:
            raise ValueError(
                f"{n_tokens} tokens need {need} pages; a row holds 1.."
                f"{self.max_blocks}")
        return need

    def _set_row(self, slot, pages):
        self._owned[slot] = pages
        self._host_table[slot, :len(pages)] = torch.tensor(
            pages, dtype=torch.int32)
        self.block_table[slot].copy_(self._host_table[slot])

    def _page_key(self, prompt_tokens, i):
        ps = self.page_size
        return tuple(prompt_tokens[i * ps:(i + 1) * ps])

    def reserve_prefix(self, slot, prompt_tokens, n_tokens):
        """reserve() that reuses cached pages for the longest registered
        prefix of prompt_tokens (a list of ints), at most (S0-1)//page_size
        pages so that at least one prompt token is computed. Returns the
        number of cached tokens, or None, changing nothing, when free plus
        evictable pages do not cover the rest."""
        if not self.prefix_cache:
            raise RuntimeError("reserve_prefix needs prefix_cache=True")
        need = self._check_reserve(slot, n_tokens)
        node, matched = self._root, []
        for i in range(min(max(len(prompt_tokens) - 1, 0) // self.page_size,
                           need)):
            node = node.children.get(self._page_key(prompt_tokens, i))
            if node is None:
                break
            matched.append(node.page)
        rest = need - len(matched)
        idle_hits = sum(1 for p in matched if self._ref[p] == 0)
        if rest > len(self._free) + len(self._idle) - idle_hits:
            return None
        # pin the matched pages before any eviction: a page with a holder is
        # not on the idle list, so it cannot be evicted for this request
        for p in matched:
            if self._ref[p] == 0:
                del self._idle[p]
            self._ref[p] += 1
        pages = list(matched)
        for _ in range(rest):
            if not self._free:
                self._evict_lru()
            p = self._free.pop()
            self._ref[p] = 1
            pages.append(p)
        self._set_row(slot, pages)
        return len(matched) * self.page_size

    def _evict_lru(self):
        """Drop the least recently used idle node and its whole subtree
        (all idle, by the refcount invariant) from the trie; their pages go
        back to the free list."""
        page = next(iter(self._idle))
        node = self._node_of[page]
        del node.parent.children[node.key]
        stack = [node]
        while stack:
            n = stack.pop()
            stack.extend(n.children.values())
            del self._node_of[n.page]
            del self._idle[n.page]
            self._free.append(n.page)
            self.evicted_pages += 1

    def publish(self, slot, prompt_tokens):
        """Register the slot's pages that prompt_tokens cover completely,
        after its prefill. Where a node already exists for a page's content
        the existing page stays registered and the slot's copy stays
        private; nothing below it is registered either, since the slot does
        not hold that node (ref(parent) >= ref(child))."""
        if not self.prefix_cache:
            raise RuntimeError("publish needs prefix_cache=True")
        pages = self._owned[slot]
        node = self._root
        for i in range(min(len(prompt_tokens) // self.page_size, len(pages))):
            key = self._page_key(prompt_tokens, i)
            child = node.children.get(key)
            if child is None:
                child = _Node(pages[i], node, key)
                node.children[key] = child
                self._node_of[pages[i]] = child
            elif child.page != pages[i]:
                break
            node = child

    def release(self, slot):
        """Return the slot's pages to the pool and reset its row to -1."""
        if not self._owned[slot]:
            raise RuntimeError(f"slot {slot} holds no pages")
        if not self.prefix_cache:
            self._free.extend(reversed(self._owned[slot]))
        else:
            # deepest page first: it becomes the older LRU entry, so a
            # prefix outlives its extensions
            for p in reversed(self._owned[slot]):
                self._ref[p] -= 1
                if self._ref[p] == 0:
                    if p in self._node_of:
                        self._idle[p] = None
                    else:
                        self._free.append(p)
        self._owned[slot] = []
        self._host_table[slot].fill_(-1)
        self.block_table[slot].copy_(self._host_table[slot])


@torch.no_grad()
def calibrate_kv_scales(model, tokens, margin=1.0):
    """Static fp8 scales from one prompt: (k_scales, v_scales), each
    [n_layers, n_kv] fp32 = max(amax, tiny) * margin / 448, where amax is
    the largest |k| (after RoPE) or |v| of that layer and kv head over the
    prompt `tokens` ([S] or [1, S] ids).

    With scale 1.0 everything below 2^-6 lands in e4m3's subnormals (step
    2^-9), which V activations commonly do; a calibrated scale puts the
    observed range at the top of the format. Values beyond the calibrated
    amax saturate at +-448 * scale (the write clamps)."""
    from kubetorch_amd import ops

    cfg = model.cfg
    tokens = torch.as_tensor(tokens, device=model.embed.weight.device)
    tokens = tokens.reshape(1, -1).long()
    S = tokens.shape[1]
    k_amax = torch.zeros(cfg.n_layers, cfg.n_kv_heads)
    v_amax = torch.zeros(cfg.n_layers, cfg.n_kv_heads)
    cos, sin = model.rope_cos[:S], model.rope_sin[:S]

    def attend(i, layer, q, k, v):
        # q [1, S, Hq, hd], k / v [1, S, n_kv, hd]
        k_amax[i] = k.float().abs().amax((0, 1, 3)).cpu()
        v_amax[i] = v.float().abs().amax((0, 1, 3)).cpu()
        o = layer.attn._sdpa(q.transpose(1, 2), k.transpose(1, 2),
                             v.transpose(1, 2), causal=True)
        return o.transpose(1, 2).reshape(1, S, -1)

    model._walk(model.embed(tokens), lambda x: ops.rope(x, cos, sin), attend)
    tiny = torch.finfo(torch.float32).tiny
    return tuple(a.clamp_min(tiny) * (margin / 448.0) for a in (k_amax, v_amax))
