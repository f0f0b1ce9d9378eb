"""Continuous-batching generation engine for the Llama family.

`Llama.generate` decodes one fixed batch to completion; a serving pod needs
requests to join and leave the batch as they arrive/finish (continuous
batching). This engine keeps a slot-per-sequence KV cache
([max_batch, n_kv, max_len, hd] per layer, plus a per-slot length vector)
and runs one batched decode step for every active slot per `step()`;
prefills fill free slots as requests arrive.

Per-slot positions make the stock forward unusable (RoPE offset and the
causal horizon differ per row). Every step here is instead the model's one
inference layer walk (`Llama._walk`, the loop behind `Llama.generate` too)
with a RoPE and an attention back-end plugged in. There are three
back-ends: the slot cache under a length mask (`_slot_math`), paged decode
(`_paged_math`) and packed paged prefill (`_prefill_math`); the prompt
forward through a throwaway KVCache is `Llama._forward_cached` itself.

`kv="paged"` (opt-in) replaces the slot slabs with a block-table paged
cache (models/paged_kv.py): pages for prompt + max_new_tokens are reserved
at admission, new k/v are scattered into pages and attention runs the
paged decode kernel (ops.paged_attention_decode), whose reads follow each
sequence's own length; one captured graph serves every horizon.

`prefill="paged"` (opt-in, needs kv="paged") runs the prompts admitted in a
step() as one packed forward straight into the pages
(ops.paged_attention_prefill): no throwaway KVCache, prompts of any lengths
share the forward, and prefill_chunk becomes packed rounds inside the same
step(). `prefix_cache=True` (implies prefill="paged") reuses the pages of
an earlier request's prompt for a new prompt that starts with the same
tokens (models/paged_kv.py); only the rest of the prompt is computed.
Lookup precedes publication, so requests admitted in the same step() do
not share pages with each other.

`kv_dtype="fp8"` (opt-in, needs kv="paged") keeps the pages as e4m3 bytes
with static fp32 scales per layer and kv head (`kv_scales`, see
models/paged_kv.py): every place that touches pages passes the layer's
scales to the paged ops, which quantise on write and dequantise on read.
Half the KV bytes per token; the allocator and the prefix cache are the
same.

`sampler="fused"` (opt-in) picks every step's tokens with one
ops.sample_tokens call over all rows (per-request temperature, top_k, top_p
and seed; a counter-based draw, so a request's tokens do not depend on its
batch mates) and one copy of the token ids to the host, in place of one
host-side `_sample` and sync per request. Under a graph the call is part of
the captured step. The default, sampler="torch", is `_sample` as it was.

`logprobs=N` (opt-in, needs sampler="fused") follows every sampler call with
one ops.token_logprobs call on the same logits rows, the returned tokens and
the rows' temperatures: the log-probability and rank of each generated token
and up to N alternatives, for the requests that ask (`submit(logprobs=n)`).
The four outputs travel to the host as one packed tensor, one copy more per
step. A finished request's record appears in `eng.logprobs[rid]`.
"""
from dataclasses import dataclass, field

import torch

from kubetorch_amd import ops


@dataclass
class _Request:
    rid: int
    prompt: torch.Tensor          # [S0] int64
    max_new_tokens: int
    temperature: float = 0.0
    stop_token: int = None
    out: list = field(default_factory=list)
    slot: int = -1
    cached_tokens: int = 0        # prompt tokens served from shared pages
    top_k: int = 0                # sampler="fused" only, as is what follows
    top_p: float = 1.0
    seed: int = 0
    logprobs: int = None          # alternatives per token; None: no record
    lp: dict = None               # the record, filled by _emit_token


class BatchedGenerator:
    def __init__(self, model, max_batch=8, max_len=None, device=None,
                 prefill_chunk=None, graph=None, kv="slot", page_size=16,
                 num_pages=None, num_splits=None, prefill="cache",
                 prefix_cache=False, kv_dtype=None, kv_scales=None,
                 sampler="torch", sampler_seed=0, logprobs=None):
        if sampler not in ("torch", "fused"):
            raise ValueError(
                f"sampler must be 'torch' or 'fused', got {sampler!r}")
        self._fused = sampler == "fused"
        self._sampler_seed = int(sampler_seed)
        if logprobs is not None:
            if not self._fused:
                raise ValueError("logprobs needs sampler='fused'")
            if not isinstance(logprobs, int) or isinstance(logprobs, bool) \
                    or not 0 <= logprobs <= ops.LOGPROBS_MAX_TOP:
                raise ValueError(
                    f"logprobs must be None or an int in "
                    f"[0, {ops.LOGPROBS_MAX_TOP}], got {logprobs!r}")
        # None: no ops.token_logprobs call anywhere; N: top_n of every call
        self._lp_n = logprobs
        # rid -> record of a finished request that asked for one (the caller
        # pops entries; the most recent 4096 rids are kept)
        self.logprobs = {}
        if kv not in ("slot", "paged"):
            raise ValueError(f"kv must be 'slot' or 'paged', got {kv!r}")
        if kv_dtype not in (None, "fp8"):
            raise ValueError(f"kv_dtype must be None or 'fp8', got {kv_dtype!r}")
        if kv_dtype == "fp8" and kv != "paged":
            raise ValueError("kv_dtype='fp8' needs kv='paged'")
        if kv_scales is not None and kv_dtype != "fp8":
            raise ValueError("kv_scales need kv_dtype='fp8'")
        k_scales, v_scales = kv_scales if kv_scales is not None \
            else (None, None)
        if prefill not in ("cache", "paged"):
            raise ValueError(
                f"prefill must be 'cache' or 'paged', got {prefill!r}")
        if (prefill == "paged" or prefix_cache) and kv != "paged":
            raise ValueError(
                "prefill='paged' and prefix_cache=True need kv='paged'")
        self._prefix = bool(prefix_cache)
        self._prefill_paged = prefill == "paged" or self._prefix
        self.prefix_stats = {"prompt_tokens": 0, "hit_tokens": 0,
                             "evicted_pages": 0}
        # rid -> prompt tokens served from the cache, most recent 4096 rids
        self.cached_tokens = {}
        self.model = model
        cfg = model.cfg
        self.cfg = cfg
        self.max_batch = max_batch
        self.prefill_chunk = prefill_chunk  # bound prefill latency spikes
        self.max_len = max_len or cfg.max_seq_len
        p = next(model.parameters())
        self.device = device or p.device
        self.dtype = p.dtype
        self._paged = kv == "paged"
        if self._paged:
            # kv="paged": block-table page pools (models/paged_kv.py) and
            # the paged HIP kernels; no slot slabs are allocated. The
            # default pool has the slot cache's capacity, so admission
            # never waits for pages; a smaller num_pages makes it wait.
            # kv_dtype="fp8" keeps that default: the same token capacity
            # in half the bytes (pass a larger num_pages to spend them).
            from kubetorch_amd.models.paged_kv import PagedKVCache

            max_blocks = -(-self.max_len // page_size)
            if num_pages is None:
                num_pages = max_batch * max_blocks
            self._pkv = PagedKVCache(cfg, num_pages, page_size, max_batch,
                                     max_blocks, self.device, self.dtype,
                                     prefix_cache=self._prefix,
                                     kv_dtype=kv_dtype, k_scales=k_scales,
                                     v_scales=v_scales)
            # fixed for the engine's life so the decode grid is static
            # (one captured graph serves every horizon)
            self._num_splits = num_splits or ops.paged_num_splits(
                max_batch, cfg.n_kv_heads, max_blocks * page_size)
        else:
            shape = (max_batch, cfg.n_kv_heads, self.max_len, cfg.head_dim)
            self.k = [torch.zeros(shape, device=self.device, dtype=self.dtype)
                      for _ in range(cfg.n_layers)]
            self.v = [torch.zeros(shape, device=self.device, dtype=self.dtype)
                      for _ in range(cfg.n_layers)]
        self.lens = torch.zeros(max_batch, dtype=torch.long, device=self.device)
        self.slots = [None] * max_batch   # slot -> _Request
        self.pending = []
        self.finished = {}
        self._next_rid = 0
        # hipGraph-captured decode step (the single-token step is
        # launch-bound: ~10 kernels x n_layers per step; one graph replay
        # removes the per-launch host cost — profiles/ROUND2.md lever 5).
        # Shape-static by construction: full max_batch every step, fixed
        # max_len horizon, static in/out buffers. KT_DECODE_GRAPH=0 or
        # graph=False forces the eager path.
        if graph is None:
            import os

            graph = (self.device.type == "cuda"
                     and os.environ.get("KT_DECODE_GRAPH", "1") != "0")
        if graph and any(hasattr(m, "ep_world") for m in model.modules()):
            graph = False  # MoE top-k dispatch is shape-dynamic: the
            # variable-size expert index_selects cannot be graph-captured
        self._use_graph = bool(graph)
        self._graphs = {}      # L bucket -> (CUDAGraph, logits buffer)
        self._g_pool = None    # shared capture mempool across buckets
        self._g_toks = None
        self._g_act = None
        self._g_rows = torch.arange(max_batch, device=self.device)
        # host mirror of per-slot lengths: picks the smallest captured
        # horizon bucket without a device sync
        self._host_lens = [0] * max_batch
        # sampler="fused": per-slot sampling parameters of the graph path
        # (static buffers, rewritten when a slot's occupant changes) and
        # the eager path's parameter rows, kept while the active set stays
        self._g_samp = None
        self._g_owner = [None] * max_batch
        self._e_samp = (None, None)

    # -- client API ----------------------------------------------------------
    def submit(self, prompt_ids, max_new_tokens=32, temperature=0.0,
               stop_token=None, top_k=0, top_p=1.0, seed=None,
               logprobs=None):
        """Queue a request; returns its id. top_k, top_p and seed need
        sampler="fused" (ops.sample_tokens has their meaning): top_k=0 and
        top_p=1.0 are off, seed=None is (sampler_seed << 32) | rid, so a
        fresh engine given the same submissions repeats its outputs. A
        request's tokens depend on its seed, never on its batch mates.

        logprobs=n (0 <= n <= the engine's logprobs=N) records, for every
        generated token, its log-probability and rank and the n most likely
        tokens with theirs (ops.token_logprobs has their meaning: the
        distribution at the request's temperature before top-k / top-p).
        When the request finishes the record is eng.logprobs[rid]: a dict
        of tokens, logprobs, ranks, top_ids and top_logprobs, one entry per
        generated token."""
        if logprobs is not None:
            if self._lp_n is None:
                raise ValueError(
                    "logprobs needs an engine built with logprobs=N")
            if not isinstance(logprobs, int) or isinstance(logprobs, bool) \
                    or not 0 <= logprobs <= self._lp_n:
                raise ValueError(
                    f"logprobs must be None or an int in [0, {self._lp_n}], "
                    f"got {logprobs!r}")
        if not self._fused:
            if top_k != 0 or top_p != 1.0 or seed is not None:
                raise ValueError(
                    "top_k, top_p and seed need sampler='fused'")
        elif not (temperature >= 0 and top_k >= 0 and 0 < top_p <= 1):
            raise ValueError("need temperature >= 0, top_k >= 0 and "
                             "0 < top_p <= 1")
        rid = self._next_rid
        self._next_rid += 1
        if seed is None:
            seed = (self._sampler_seed << 32) | rid
        seed = (int(seed) + 2 ** 63) % 2 ** 64 - 2 ** 63   # as int64
        prompt = torch.as_tensor(prompt_ids, dtype=torch.long,
                                 device=self.device).reshape(-1)
        if prompt.numel() + max_new_tokens > self.max_len:
            raise ValueError("prompt + max_new_tokens exceeds max_len")
        if self._paged and self._pkv.pages_needed(
                prompt.numel() + max_new_tokens) > self._pkv.num_pages:
            raise ValueError("request needs more pages than the pool holds")
        self.pending.append(_Request(rid, prompt, max_new_tokens,
                                     temperature, stop_token,
                                     top_k=int(top_k), top_p=float(top_p),
                                     seed=seed, logprobs=logprobs))
        return rid

    @property
    def has_work(self):
        return bool(self.pending) or any(s is not None for s in self.slots)

    def run(self):
        """Drive to completion; returns {rid: token list (prompt + new)}."""
        while self.has_work:
            self.step()
        out, self.finished = self.finished, {}
        return out

    # -- engine --------------------------------------------------------------
    @torch.no_grad()
    def step(self):
        """One engine iteration: admit pending prompts into free slots
        (prefill — same-length prompts share one batched forward), then
        one batched decode step for every active slot."""
        admitted = []
        for slot in range(self.max_batch):
            if self.slots[slot] is None and self.pending:
                if self._paged:
                    # FIFO: if the head does not fit, it and everything
                    # behind it wait for pages freed by a later finish
                    head = self.pending[0]
                    n = head.prompt.numel() + head.max_new_tokens
                    if self._prefix:
                        hit = self._pkv.reserve_prefix(
                            slot, head.prompt.tolist(), n)
                        if hit is None:
                            break
                        head.cached_tokens = hit
                        self.cached_tokens[head.rid] = hit
                        if len(self.cached_tokens) > 4096:
                            del self.cached_tokens[next(iter(
                                self.cached_tokens))]
                        self.prefix_stats["prompt_tokens"] += \
                            head.prompt.numel()
                        self.prefix_stats["hit_tokens"] += hit
                        self.prefix_stats["evicted_pages"] = \
                            self._pkv.evicted_pages
                    elif not self._pkv.reserve(slot, n):
                        break
                req = self.pending.pop(0)
                req.slot = slot
                self.slots[slot] = req
                admitted.append(req)
        if admitted and self._prefill_paged:
            self._prefill_packed(admitted)
        elif admitted:
            by_len = {}
            for req in admitted:
                by_len.setdefault(req.prompt.numel(), []).append(req)
            for group in by_len.values():
                # chunked prefill stays one request at a time
                for g in ([[r] for r in group] if self.prefill_chunk
                          else [group]):
                    self._prefill(g)
        active = [s for s in range(self.max_batch) if self.slots[s] is not None]
        if active:
            self._decode(active)

    def _prefill(self, group):
        """Run G same-length prompts through one throwaway KVCache, in
        prefill_chunk-token pieces if set, then move each row's KV into its
        request's slot. (A 1-at-a-time prefill is GEMM-starved: [1, S0]
        activations; [G, S0] runs the same layer GEMMs at G-fold
        arithmetic intensity.)"""
        from kubetorch_amd.models.llama import KVCache

        S0 = group[0].prompt.numel()
        batch = (torch.stack([req.prompt for req in group])
                 if len(group) > 1 else group[0].prompt.view(1, -1))
        cache = KVCache(self.cfg, len(group), S0, self.device, self.dtype)
        pc = self.prefill_chunk
        chunk = pc if pc and pc < S0 else S0
        for s0 in range(0, S0, chunk):
            logits = self.model._forward_cached(batch[:, s0:s0 + chunk],
                                                cache)
        toks, recs = self._sample_rows(group, logits) if self._fused \
            else (None, None)
        for j, req in enumerate(group):
            self._store_prefill(req, cache, j, S0)
            self.lens[req.slot] = S0
            self._host_lens[req.slot] = S0
            req.out = req.prompt.tolist()
            if toks is None:
                self._emit(req, logits[j])
            else:
                self._emit_token(req, toks[j], recs and recs[j])

    def _store_prefill(self, req, cache, j, S0):
        """Move row j of a prefill cache into the request's slot (slot
        mode) or scatter it into the slot's pages (paged mode: one
        paged_kv_write per layer)."""
        if not self._paged:
            for i in range(self.cfg.n_layers):
                self.k[i][req.slot, :, :S0] = cache.k[i][j, :, :S0]
                self.v[i][req.slot, :, :S0] = cache.v[i][j, :, :S0]
            return
        slot_map = torch.tensor(self._pkv.token_slots(req.slot, 0, S0),
                                dtype=torch.int32).to(self.device)
        for i in range(self.cfg.n_layers):
            # [n_kv, S0, hd] -> [S0, n_kv, hd] views, no copy; fp8 pools
            # quantise the rows on their way in (scales None otherwise)
            ops.paged_kv_write(cache.k[i][j, :, :S0].transpose(0, 1),
                               cache.v[i][j, :, :S0].transpose(0, 1),
                               self._pkv.k[i], self._pkv.v[i], slot_map,
                               self._pkv.k_scale[i], self._pkv.v_scale[i])

    def _prefill_packed(self, reqs):
        """Prefill every admitted request in packed forwards over the pages:
        each round takes the next tokens of every unfinished prompt (all of
        them, or at most prefill_chunk per request), whatever the lengths.
        Tokens served by the prefix cache are skipped; a request whose
        prompt is in gets its first token from the round's logits."""
        pc = self.prefill_chunk
        done = {r.rid: r.cached_tokens for r in reqs}
        todo = list(reqs)
        while todo:
            toks, pos, slot_map, cu, seq_lens, last = [], [], [], [0], [], []
            for r in todo:
                d0, S0 = done[r.rid], r.prompt.numel()
                n = min(S0 - d0, pc) if pc else S0 - d0
                toks.append(r.prompt[d0:d0 + n])
                pos.extend(range(d0, d0 + n))
                slot_map.extend(self._pkv.token_slots(r.slot, d0, d0 + n))
                cu.append(cu[-1] + n)
                seq_lens.append(d0 + n)
                last.append(cu[-1] - 1)
                done[r.rid] = d0 + n
            dev = self.device
            i32 = torch.int32
            logits = self._prefill_math(
                torch.cat(toks), torch.tensor(pos).to(dev),
                torch.tensor(slot_map, dtype=i32).to(dev),
                self._pkv.block_table[torch.tensor(
                    [r.slot for r in todo]).to(dev)],
                torch.tensor(cu, dtype=i32).to(dev),
                torch.tensor(seq_lens, dtype=i32).to(dev),
                max(b - a for a, b in zip(cu, cu[1:])),
                torch.tensor(last).to(dev))
            rest = []
            toks, recs = {}, None
            if self._fused:  # one call for the rows whose prompt is in
                fin = [j for j, r in enumerate(todo)
                       if done[r.rid] >= r.prompt.numel()]
                if fin:
                    rows = logits if len(fin) == len(todo) else \
                        logits[torch.tensor(fin).to(dev)]
                    picked, recs = self._sample_rows(
                        [todo[j] for j in fin], rows)
                    toks = dict(zip(fin, picked))
                    recs = recs and dict(zip(fin, recs))
            for j, r in enumerate(todo):
                S0 = r.prompt.numel()
                if done[r.rid] < S0:
                    rest.append(r)
                    continue
                self.lens[r.slot] = S0
                self._host_lens[r.slot] = S0
                r.out = r.prompt.tolist()
                if self._prefix:  # before _emit, which may release the slot
                    self._pkv.publish(r.slot, r.out)
                if self._fused:
                    self._emit_token(r, toks[j], recs and recs[j])
                else:
                    self._emit(r, logits[j])
            todo = rest

    def _prefill_math(self, toks, pos, slot_map, table, cu, seq_lens, max_q,
                      last):
        """One packed prefill forward over the paged cache, in the style of
        _paged_math: toks/pos/slot_map [T] are the packed tokens, their
        positions and physical slots; row j of table/seq_lens and cu[j],
        cu[j+1] describe request j. New k/v go to their pages before
        attention reads them. Returns logits [len(last), vocab] of the
        packed tokens `last`."""
        m = self.model
        T = toks.shape[0]
        cos = m.rope_cos[pos]
        sin = m.rope_sin[pos]

        def attend(i, layer, q, k, v):
            kp, vp = self._pkv.k[i], self._pkv.v[i]
            ks, vs = self._pkv.k_scale[i], self._pkv.v_scale[i]
            ops.paged_kv_write(k[0], v[0], kp, vp, slot_map, ks, vs)
            o = ops.paged_attention_prefill(q[0], kp, vp, table, cu,
                                            seq_lens, max_q, k_scale=ks,
                                            v_scale=vs)
            return o.reshape(1, T, -1)

        h = m._walk(m.embed(toks.view(1, T)),
                    lambda x: ops.rope(x, cos, sin), attend)
        return m._head(h[:, last])[0]

    def _sample(self, req, logits):
        if req.temperature > 0:
            probs = torch.softmax(logits.float() / req.temperature, -1)
            return int(torch.multinomial(probs, 1))
        return int(logits.argmax(-1))

    # -- sampler="fused": ops.sample_tokens over all rows of a step ----------
    @staticmethod
    def _generated(req):
        """Tokens the request has generated so far = its next draw's
        offset (0 for the token that comes out of prefill)."""
        return max(0, len(req.out) - req.prompt.numel())

    def _sample_params(self, reqs):
        """The five [len(reqs)] parameter vectors of ops.sample_tokens on
        the device; None entries (free graph slots) are greedy rows."""
        rows = [(r.temperature, r.top_k, r.top_p, r.seed, self._generated(r))
                if r is not None else (0.0, 0, 1.0, 0, 0) for r in reqs]
        t, k, p, sd, off = zip(*rows)
        dev = self.device
        return [torch.tensor(t, dtype=torch.float32).to(dev),
                torch.tensor(k, dtype=torch.int32).to(dev),
                torch.tensor(p, dtype=torch.float32).to(dev),
                torch.tensor(sd, dtype=torch.int64).to(dev),
                torch.tensor(off, dtype=torch.int64).to(dev)]

    def _sample_rows(self, reqs, logits):
        """Row j of logits [len(reqs), vocab] is request j's: one sampler
        call and one copy to the host -> (list of token ids, the rows'
        log-prob records or None when no request of the call asked)."""
        params = self._sample_params(reqs)
        toks = ops.sample_tokens(logits, *params)
        recs = None
        if self._wants_logprobs(reqs):
            recs = self._logprob_rows(logits, toks, params[0]).tolist()
        return toks.tolist(), recs

    # -- logprobs=N: ops.token_logprobs after every sampler call -------------
    def _wants_logprobs(self, reqs):
        return self._lp_n is not None and any(
            r is not None and r.logprobs is not None for r in reqs)

    def _logprob_rows(self, logits, toks, temperature):
        """ops.token_logprobs on the rows a sampler call saw and the tokens
        it returned, packed for one copy to the host: row j is float64
        [logprob, rank, N top ids, N top log-probs] (fp32 and int32 values
        are exact in float64). Capturable."""
        lp, rank, ids, top = ops.token_logprobs(logits, toks, temperature,
                                                self._lp_n)
        B = lp.shape[0]
        return torch.cat([lp.double().view(B, 1), rank.double().view(B, 1),
                          ids.double(), top.double()], dim=1)

    def _emit(self, req, logits):
        self._emit_token(req, self._sample(req, logits))

    def _emit_token(self, req, nxt, rec=None):
        """Append token nxt to the request; rec is its packed row of
        _logprob_rows, of which a request that asked keeps its own n
        alternatives."""
        req.out.append(nxt)
        req.next_tok = nxt
        if req.logprobs is not None:
            if req.lp is None:
                req.lp = {"tokens": [], "logprobs": [], "ranks": [],
                          "top_ids": [], "top_logprobs": []}
            n, N = req.logprobs, self._lp_n
            req.lp["tokens"].append(nxt)
            req.lp["logprobs"].append(rec[0])
            req.lp["ranks"].append(int(rec[1]))
            req.lp["top_ids"].append([int(i) for i in rec[2:2 + n]])
            req.lp["top_logprobs"].append(rec[2 + N:2 + N + n])
        done = (len(req.out) - req.prompt.numel() >= req.max_new_tokens
                or (req.stop_token is not None and nxt == req.stop_token))
        if done:
            self.finished[req.rid] = req.out
            if req.lp is not None:
                self.logprobs[req.rid] = req.lp
                if len(self.logprobs) > 4096:
                    del self.logprobs[next(iter(self.logprobs))]
            self.slots[req.slot] = None
            self.lens[req.slot] = 0
            self._host_lens[req.slot] = 0
            if self._paged:
                self._pkv.release(req.slot)

    def _decode(self, active):
        if self._use_graph:
            return self._decode_graph(active)
        return self._decode_eager(active)

    # -- decode maths (capturable: no host syncs, no data-dependent flow) -----
    def _decode_walk(self, toks, lens, attend):
        """One single-token step for B rows at per-row positions `lens`:
        the model's layer walk with per-row RoPE tables (fp32) and the
        cache's `attend`; returns logits [B, vocab]."""
        m = self.model
        B = toks.shape[0]
        half = self.cfg.head_dim // 2
        cos = m.rope_cos[lens].view(B, 1, 1, half)
        sin = m.rope_sin[lens].view(B, 1, 1, half)
        h = m._walk(m.embed(toks).view(B, 1, -1),
                    lambda x: self._rope1(x, cos, sin), attend)
        return m._head(h)[:, -1]

    def _slot_math(self, toks, lens, L, idx=None):
        """One decode step over the slot cache, horizon L: new k/v go to
        each row's own position and SDPA runs under a length mask (row b
        sees [0, lens[b]]). idx=None is every slot, read as the view
        [:, :, :L] (the graph path: fixed shapes, no gather of the cache);
        inactive slots then decode garbage (their mask exposes only cache
        row 0), are ignored at emit time, and their cache rows are
        overwritten by the next prefill. With idx, toks/lens belong to
        those slots and the cache rows are gathered."""
        B = toks.shape[0]
        rows = self._g_rows if idx is None else idx
        ar = torch.arange(L, device=self.device)
        mask = (ar.view(1, L) <= lens.view(B, 1)).view(B, 1, 1, L)

        def attend(i, layer, q, k, v):
            # advanced indexing: [rows, :, lens] -> [B, n_kv, hd] rows
            self.k[i][rows, :, lens] = k[:, 0]
            self.v[i][rows, :, lens] = v[:, 0]
            if idx is None:
                kf, vf = self.k[i][:, :, :L], self.v[i][:, :, :L]
            else:
                kf, vf = self.k[i][idx, :, :L], self.v[i][idx, :, :L]
            o = layer.attn._sdpa(q.transpose(1, 2), kf, vf, mask=mask)
            return o.transpose(1, 2).reshape(B, 1, -1)

        return self._decode_walk(toks, lens, attend)

    def _paged_math(self, toks, lens, act, table):
        """One decode step over the paged cache for the rows given (all
        slots under a graph, the active ones in eager mode): same math as
        the slot step, but new k/v go to their pages with paged_kv_write
        and attention is ops.paged_attention_decode, which reads lengths
        and tables from device buffers. No mask tensor, no horizon slice,
        no host sync. Rows with act == 0 write nothing (negative slot) and
        attend over nothing (length 0, zero output)."""
        B = toks.shape[0]
        ps = self._pkv.page_size
        blk = (lens // ps).clamp(max=self._pkv.max_blocks - 1)
        page = table.gather(1, blk.view(B, 1)).view(B).long()
        live = (act > 0) & (page >= 0)
        slot_map = torch.where(live, page * ps + lens % ps,
                               torch.full_like(page, -1)).to(torch.int32)
        seq_lens = ((lens + 1) * act).to(torch.int32)

        def attend(i, layer, q, k, v):
            kp, vp = self._pkv.k[i], self._pkv.v[i]
            ks, vs = self._pkv.k_scale[i], self._pkv.v_scale[i]
            ops.paged_kv_write(k[:, 0], v[:, 0], kp, vp, slot_map, ks, vs)
            o = ops.paged_attention_decode(q[:, 0], kp, vp, table, seq_lens,
                                           num_splits=self._num_splits,
                                           k_scale=ks, v_scale=vs)
            return o.reshape(B, 1, -1)

        return self._decode_walk(toks, lens, attend)

    # -- hipGraph path -------------------------------------------------------
    def _decode_math(self, L=None):
        """One full-batch decode step as a pure function of the static
        buffers (_g_toks, lens, _g_act), which is what a graph captures:
        over horizon L of the slot cache, or over the pages (no L)."""
        if self._paged:
            logits = self._paged_math(self._g_toks, self.lens, self._g_act,
                                      self._pkv.block_table)
        else:
            logits = self._slot_math(self._g_toks, self.lens, L)
        self.lens.add_(self._g_act)  # active slots advance one position
        if self._fused:
            # the step's tokens [max_batch] instead of its logits; free
            # slots are greedy rows over garbage and are ignored
            toks = ops.sample_tokens(logits, *self._g_samp)
            self._g_samp[4].add_(self._g_act)  # offset: one more drawn
            if self._lp_n is not None:
                # always part of the step, whoever asked: the captured graph
                # is one for the engine's life
                return toks, self._logprob_rows(logits, toks,
                                                self._g_samp[0])
            return toks
        return logits

    def _bucket_for(self, need):
        """Smallest power-of-two horizon >= need (>=128), capped at
        max_len. The per-bucket graphs keep attention reads proportional
        to the actual active horizon instead of the full cache."""
        L = 128
        while L < need:
            L *= 2
        return min(L, self.max_len)

    def _ensure_graph(self, L):
        g = self._graphs.get(L)
        if g is not None:
            return g
        if self._g_toks is None:
            self._g_toks = torch.zeros(self.max_batch, dtype=torch.long,
                                       device=self.device)
            self._g_act = torch.zeros(self.max_batch, dtype=torch.long,
                                      device=self.device)
            self._g_pool = torch.cuda.graph_pool_handle()
            if self._fused:
                self._g_samp = self._sample_params([None] * self.max_batch)
        lens_snapshot = self.lens.clone()
        off_snapshot = self._g_samp[4].clone() if self._fused else None
        horizon = None if self._paged else L
        for _ in range(2):  # warm up allocator/workspaces pre-capture
            self._decode_math(horizon)
        self.lens.copy_(lens_snapshot)
        if self._fused:
            self._g_samp[4].copy_(off_snapshot)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, pool=self._g_pool):
            logits = self._decode_math(horizon)
        self._graphs[L] = (graph, logits)
        return self._graphs[L]

    def _decode_graph(self, active):
        if self._paged:
            # one graph for every horizon: the kernel takes lengths and
            # block tables from device memory, and its grid is static
            graph, logits = self._ensure_graph("paged")
        else:
            need = max(self._host_lens[s] for s in active) + 1
            graph, logits = self._ensure_graph(self._bucket_for(need))
        toks = [0] * self.max_batch
        act = [0] * self.max_batch
        for s in active:
            toks[s] = self.slots[s].next_tok
            act[s] = 1
            self._host_lens[s] += 1
        self._g_toks.copy_(torch.tensor(toks, dtype=torch.long),
                           non_blocking=True)
        self._g_act.copy_(torch.tensor(act, dtype=torch.long),
                          non_blocking=True)
        if self._fused:
            owner = [r.rid if r is not None else None for r in self.slots]
            if owner != self._g_owner:  # a slot's occupant changed
                for buf, new in zip(self._g_samp,
                                    self._sample_params(self.slots)):
                    buf.copy_(new, non_blocking=True)
                self._g_owner = owner
            graph.replay()
            recs = None
            if self._lp_n is not None:  # the output is (tokens, records)
                logits, packed = logits
                if self._wants_logprobs(self.slots):
                    recs = packed.tolist()
            toks = logits.tolist()  # the graph's output is the tokens
            for s in active:
                self._emit_token(self.slots[s], toks[s], recs and recs[s])
            return
        graph.replay()
        for s in active:
            self._emit(self.slots[s], logits[s])

    # -- eager path (CPU, or KT_DECODE_GRAPH=0) ------------------------------
    def _decode_eager(self, active):
        idx = torch.tensor(active, device=self.device)
        toks = torch.tensor([self.slots[s].next_tok for s in active],
                            device=self.device)
        lens = self.lens[idx]                      # position of the new token
        if self._paged:
            logits = self._paged_math(toks, lens, torch.ones_like(idx),
                                      self._pkv.block_table[idx])
        else:
            # longest horizon this step (a host sync)
            logits = self._slot_math(toks, lens, int(lens.max().item()) + 1,
                                     idx)
        self.lens[idx] += 1
        if self._fused:
            # the parameter rows stay on the device while the same requests
            # are active; only their offsets move, one draw per step
            rids = [self.slots[s].rid for s in active]
            if self._e_samp[0] != rids:
                self._e_samp = (rids, self._sample_params(
                    [self.slots[s] for s in active]))
            params = self._e_samp[1]
            toks = ops.sample_tokens(logits, *params)
            params[4] += 1
            recs = None
            if self._wants_logprobs([self.slots[s] for s in active]):
                recs = self._logprob_rows(logits, toks, params[0]).tolist()
            toks = toks.tolist()
            for j, s in enumerate(active):
                self._emit_token(self.slots[s], toks[j], recs and recs[j])
            return
        for j, s in enumerate(active):
            self._emit(self.slots[s], logits[j])

    @staticmethod
    def _rope1(x, cos, sin):
        # single-position rotate-half, per-row tables (fp32 math, same
        # formula as ops._rope_ref so numerics match the prefill path)
        D = x.shape[-1]
        xf = x.float()
        x1, x2 = xf[..., :D // 2], xf[..., D // 2:]
        o1 = x1 * cos - x2 * sin
        o2 = x2 * cos + x1 * sin
        return torch.cat([o1, o2], dim=-1).to(x.dtype)
