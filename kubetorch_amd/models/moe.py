"""Mixture-of-Experts MLP for the Llama family (Mixtral-style top-k).

Routing + dispatch is torch (memory-bound gather/scatter); each expert's
FFN uses the same fused SwiGLU op as the dense MLP. Two placements:

  * dense (default): all experts on every rank — token-grouped batched
    expert GEMMs, DP-compatible as-is.
  * expert parallel (ep_group): experts sharded across the group's ranks.
    The EP group is sequence-replicated (every rank in it runs the same
    tokens — the TP-style placement; compose with DP ACROSS groups, not
    inside one): each rank computes its local experts and the partial
    outputs are all-reduce summed. Correct on any backend (gloo CI
    included); the all_to_all token exchange for data-sharded EP (less
    traffic when top_k << n_experts/world) is a round-2 swap kept behind
    the same interface.

FusedMoEMLP / fuse_moe are the single-rank inference form of the same
block: the experts' weights stacked into two parameters and the whole MLP
one ops.moe_mlp call, which at decode sizes (at most 32 tokens) runs the
gfx950 routed-GEMM kernels without a host sync, so the serving engine keeps
its captured decode graph, and above that (prefill, wide decode steps) the
gfx950 grouped-GEMM kernels, again without a host sync.

The reference ships no model code — this extends the
flagship family the launchers run, and is the EP workload the SPMD
launcher's process groups exist for.
"""
import copy

import torch
import torch.nn as nn
import torch.nn.functional as F

from kubetorch_amd import ops


class Expert(nn.Module):
    def __init__(self, dim, intermediate):
        super().__init__()
        self.w_gate_up = nn.Linear(dim, 2 * intermediate, bias=False)
        self.w_down = nn.Linear(intermediate, dim, bias=False)

    def forward(self, x):
        return self.w_down(ops.swiglu(self.w_gate_up(x)))


class MoEMLP(nn.Module):
    """Drop-in replacement for the dense MLP block.

    n_experts total experts, top_k per token, softmax-normalized over the
    selected k (Mixtral convention). With ep_group, rank r owns experts
    [r*n_local, (r+1)*n_local).
    """

    def __init__(self, cfg, n_experts=8, top_k=2, ep_group=None):
        super().__init__()
        import torch.distributed as dist

        self.dim = cfg.dim
        self.n_experts = n_experts
        self.top_k = top_k
        self.router = nn.Linear(cfg.dim, n_experts, bias=False)
        self.ep_group = ep_group
        if ep_group is not None and dist.is_initialized():
            self.ep_world = dist.get_world_size(ep_group)
            self.ep_rank = dist.get_rank(ep_group)
        else:
            self.ep_world, self.ep_rank = 1, 0
        if n_experts % self.ep_world:
            raise ValueError("n_experts must divide by the EP world size")
        self.n_local = n_experts // self.ep_world
        self.local_offset = self.ep_rank * self.n_local
        self.experts = nn.ModuleList(
            Expert(cfg.dim, cfg.intermediate) for _ in range(self.n_local))

    def forward(self, x):
        B, S, D = x.shape
        flat = x.reshape(-1, D)
        logits = self.router(flat)                         # [T, E]
        weights, sel = logits.topk(self.top_k, dim=-1)     # [T, k]
        weights = torch.softmax(weights.float(), dim=-1).to(x.dtype)
        if self.ep_world == 1:
            out = self._dispatch_local(flat, sel, weights, base=0)
        else:
            out = self._dispatch_ep(flat, sel, weights)
        return out.reshape(B, S, D)

    def _dispatch_local(self, flat, sel, weights, base, out=None):
        """Compute this module's experts for their assigned tokens and
        weighted-scatter into out. base maps local expert i -> global id."""
        if out is None:
            out = torch.zeros_like(flat)
        for i, expert in enumerate(self.experts):
            eid = base + i
            tok, kth = (sel == eid).nonzero(as_tuple=True)  # tokens; which k
            if tok.numel() == 0:
                continue
            y = expert(flat[tok])
            out.index_add_(0, tok, y * weights[tok, kth].unsqueeze(-1))
        return out

    def _dispatch_ep(self, flat, sel, weights):
        """Sequence-replicated EP: every rank in the group runs the same
        tokens (router weights identical across the group), computes only
        its local experts, then the partial outputs are summed."""
        import torch.distributed as dist

        out = self._dispatch_local(flat, sel, weights, base=self.local_offset)
        dist.all_reduce(out, op=dist.ReduceOp.SUM, group=self.ep_group)
        return out

    def aux_load_balance_loss(self, x):
        """Switch-style load-balance auxiliary loss (fraction-of-tokens x
        mean-router-prob per expert, scaled by n_experts)."""
        flat = x.reshape(-1, self.dim)
        probs = torch.softmax(self.router(flat).float(), dim=-1)   # [T, E]
        _, sel = probs.topk(self.top_k, dim=-1)
        counts = torch.zeros(self.n_experts, device=x.device)
        counts.scatter_add_(0, sel.reshape(-1),
                            torch.ones(sel.numel(), device=x.device))
        frac = counts / max(1, sel.numel())
        return self.n_experts * (frac * probs.mean(0)).sum()


def _init_linear(linear, std, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        w = torch.empty(linear.weight.shape, dtype=torch.float32)
        w.normal_(0.0, std, generator=g)
        linear.weight.copy_(w.to(linear.weight.dtype))


def convert_to_moe(model, n_experts=8, top_k=2, ep_group=None, seed=0):
    """Swap every Block's dense MLP for a MoEMLP. Weights are seeded per
    GLOBAL expert id, so every EP sharding of the same (seed, n_experts)
    holds identical experts — a 2-rank EP run computes exactly what the
    single-rank dense placement computes (tested)."""
    std = model.cfg.init_std
    p = next(model.parameters())
    for li, layer in enumerate(model.layers):
        moe = MoEMLP(model.cfg, n_experts=n_experts, top_k=top_k,
                     ep_group=ep_group)
        _init_linear(moe.router, std, seed * 100003 + li)
        for i, ex in enumerate(moe.experts):
            gid = moe.local_offset + i
            _init_linear(ex.w_gate_up, std,
                         seed * 100003 + li * 1009 + gid * 2 + 7)
            _init_linear(ex.w_down, std,
                         seed * 100003 + li * 1009 + gid * 2 + 8)
        layer.mlp = moe.to(device=p.device, dtype=p.dtype)
    return model


class FusedMoEMLP(nn.Module):
    """Inference form of a single-rank MoEMLP: `router` and the experts'
    weights stacked as w_gate_up [E, 2I, D] and w_down [E, D, I]; forward is
    the router followed by ops.moe_mlp.

    A numerical contract of its own, not bit-equal to MoEMLP: the routing
    weights stay fp32, the top-k sum is carried in fp32 and rounded once, and
    h = silu(gate) * up is rounded once from fp32 (MoEMLP rounds the routing
    weights, gate/up, each expert's output and every partial sum to the
    model's dtype). Equal router logits go to the lowest expert index.

    quantize_fp8_() turns the two weights into e4m3 buffers of the same names
    with fp32 buffers w_gate_up_scale [E, 2I] and w_down_scale [E, D]
    (ops.quantize_weight_fp8 per expert); a dtype cast of the model then
    leaves them as they are, device moves apply."""

    # The rows of ops.moe_mlp's decode kernels. Calls of more rows run its
    # grouped kernels (no host sync either); the serving engine still captures
    # no decode graph above this.
    graph_max_rows = ops.MOE_MAX_ROWS

    def __init__(self, dim, intermediate, n_experts=8, top_k=2, device=None,
                 dtype=None):
        super().__init__()
        if not 1 <= top_k <= n_experts:
            raise ValueError("top_k must be in [1, n_experts]")
        self.dim = dim
        self.intermediate = intermediate
        self.n_experts = n_experts
        self.top_k = top_k
        kw = dict(device=device, dtype=dtype)
        self.router = nn.Linear(dim, n_experts, bias=False, **kw)
        self.w_gate_up = nn.Parameter(
            torch.zeros(n_experts, 2 * intermediate, dim, **kw))
        self.w_down = nn.Parameter(
            torch.zeros(n_experts, dim, intermediate, **kw))

    @classmethod
    @torch.no_grad()
    def from_moe(cls, moe):
        """The fused module that holds a single-rank MoEMLP's weights."""
        if getattr(moe, "ep_world", 1) > 1:
            raise ValueError("FusedMoEMLP is single-rank: the MoEMLP is "
                             f"sharded over {moe.ep_world} ranks")
        w = moe.router.weight
        inter = moe.experts[0].w_down.weight.shape[1]
        new = cls(moe.dim, inter, moe.n_experts, moe.top_k, device="meta")
        new.router.weight = nn.Parameter(w.detach().clone())
        new.w_gate_up = nn.Parameter(torch.stack(
            [ex.w_gate_up.weight.detach() for ex in moe.experts]))
        new.w_down = nn.Parameter(torch.stack(
            [ex.w_down.weight.detach() for ex in moe.experts]))
        return new

    @property
    def is_fp8(self):
        return self.w_gate_up.dtype == ops.W8_DTYPE

    @torch.no_grad()
    def quantize_fp8_(self):
        """Quantise the experts' weights in place, expert by expert (the fp32
        temporary is one expert's matrix); each bf16 tensor is dropped as
        soon as its replacement exists. The scale values are validated here,
        once, on the host."""
        if self.is_fp8:
            return self
        for name in ("w_gate_up", "w_down"):
            w = getattr(self, name)
            q = torch.empty(w.shape, dtype=ops.W8_DTYPE, device=w.device)
            scale = torch.empty(w.shape[:2], dtype=torch.float32,
                                device=w.device)
            for e in range(w.shape[0]):
                q[e], scale[e] = ops.quantize_weight_fp8(w[e])
            self.set_fp8_(name, q, scale)
        return self

    def set_fp8_(self, name, q, scale):
        """Install e4m3 bytes q [E, N, K] and their row scales [E, N] as the
        buffers `name` and `name`_scale, replacing the parameter."""
        if q.dtype != ops.W8_DTYPE or scale.dtype != torch.float32 \
                or tuple(scale.shape) != tuple(q.shape[:2]):
            raise ValueError(f"{name}: expected e4m3 [E, N, K] and fp32 "
                             "[E, N] scales")
        ops._check_w8_scale_values(scale)
        self._parameters.pop(name, None)
        self._buffers.pop(name, None)
        self._buffers.pop(name + "_scale", None)
        self.register_buffer(name, q.contiguous())
        self.register_buffer(name + "_scale", scale.contiguous())

    def _apply(self, fn, recurse=True):
        # device moves apply; dtype casts must not touch the fp8 bytes or
        # round the scales
        if not self.is_fp8:
            return super()._apply(fn, recurse)
        names = ("w_gate_up", "w_down", "w_gate_up_scale", "w_down_scale")
        old = {n: getattr(self, n) for n in names}
        super()._apply(fn, recurse)
        for n, t in old.items():
            new = getattr(self, n)
            if new.dtype != t.dtype:
                setattr(self, n, t.to(new.device))
        return self

    def forward(self, x):
        if self.is_fp8:
            return ops.moe_mlp(x, self.router(x), self.w_gate_up, self.w_down,
                               self.top_k,
                               w_gate_up_scale=self.w_gate_up_scale,
                               w_down_scale=self.w_down_scale)
        return ops.moe_mlp(x, self.router(x), self.w_gate_up, self.w_down,
                           self.top_k)

    def extra_repr(self):
        return (f"dim={self.dim}, intermediate={self.intermediate}, "
                f"n_experts={self.n_experts}, top_k={self.top_k}"
                + (", weight=e4m3" if self.is_fp8 else ""))


def fuse_moe(model, inplace=False):
    """Replace every MoEMLP of `model` with a FusedMoEMLP holding the same
    weights (inference only). inplace=False works on a deep copy and leaves
    `model` as it is. A model sharded by expert parallelism (ep_world > 1)
    raises ValueError. Returns the fused model."""
    from kubetorch_amd.models.quantize import _swap

    for m in model.modules():
        if isinstance(m, MoEMLP) and m.ep_world > 1:
            raise ValueError("fuse_moe needs a single-rank model: a MoEMLP "
                             f"is sharded over {m.ep_world} ranks")
    if not inplace:
        model = copy.deepcopy(model)
    _swap(model, lambda m: isinstance(m, MoEMLP),
          lambda name, m: FusedMoEMLP.from_moe(m))
    return model
