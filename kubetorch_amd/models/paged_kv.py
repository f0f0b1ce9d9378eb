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
"""
import torch


class PagedKVCache:
    def __init__(self, cfg, num_pages, page_size, max_batch, max_blocks,
                 device, dtype):
        if num_pages < 1 or max_blocks < 1 or max_batch < 1:
            raise ValueError("num_pages, max_blocks and max_batch must be >= 1")
        self.num_pages = num_pages
        self.page_size = page_size
        self.max_batch = max_batch
        self.max_blocks = max_blocks
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

    @property
    def free_pages(self):
        return len(self._free)

    def pages_of(self, slot):
        return list(self._owned[slot])

    def pages_needed(self, n_tokens):
        return -(-n_tokens // self.page_size)

    def reserve(self, slot, n_tokens):
        """Give `slot` the pages for n_tokens tokens and fill its table row.
        Returns False, changing nothing, when not enough pages are free."""
        if self._owned[slot]:
            raise RuntimeError(f"slot {slot} already holds pages")
        need = self.pages_needed(n_tokens)
        if need < 1 or need > self.max_blocks:
            raise ValueError(
                f"{n_tokens} tokens need {need} pages; a row holds 1.."
                f"{self.max_blocks}")
        if need > len(self._free):
            return False
        pages = [self._free.pop() for _ in range(need)]
        self._owned[slot] = pages
        self._host_table[slot, :need] = torch.tensor(pages, dtype=torch.int32)
        self.block_table[slot].copy_(self._host_table[slot])
        return True

    def release(self, slot):
        """Return the slot's pages to the pool and reset its row to -1."""
        if not self._owned[slot]:
            raise RuntimeError(f"slot {slot} holds no pages")
        self._free.extend(reversed(self._owned[slot]))
        self._owned[slot] = []
        self._host_table[slot].fill_(-1)
        self.block_table[slot].copy_(self._host_table[slot])
