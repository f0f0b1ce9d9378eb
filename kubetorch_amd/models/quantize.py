"""FP8 weight-only quantisation of a model's ops.Linear layers and of its
fused MoE experts (FusedMoEMLP).

quantize_weights_fp8 swaps every ops.Linear (wqkv, wo, w_gate_up, w_down,
lm_head of a Llama) for ops.LinearW8; the model's walk, generate() and
BatchedGenerator call the modules and run unchanged. dequantize_weights is
the way back: the same model with plain ops.Linear layers that hold the
matrix the fp8 layers represent, which is exactly representable in bf16.
"""
import copy

import torch

from kubetorch_amd import ops
from kubetorch_amd.models.moe import FusedMoEMLP


def _swap(model, match, make):
    """Replace every child module m with match(m) by make(qualified name, m);
    returns the number replaced."""
    n = 0
    for pname, parent in list(model.named_modules()):
        for cname, child in list(parent.named_children()):
            if match(child):
                new = make(f"{pname}.{cname}" if pname else cname, child)
                if new is not None:
                    setattr(parent, cname, new)
                    n += 1
    return n


@torch.no_grad()
def quantize_weights_fp8(model, skip=(), inplace=False):
    """Replace every ops.Linear of `model` with ops.LinearW8 holding its
    weight as e4m3 bytes and one power-of-two fp32 scale per output row
    (ops.quantize_weight_fp8). Modules whose qualified name ends in an entry
    of `skip` (e.g. "lm_head") are left alone; embeddings, norms and plain
    nn.Linear layers (unfused MoE experts, every router) are never touched.
    A FusedMoEMLP keeps its class: its w_gate_up and w_down become e4m3
    buffers with fp32 row scales (FusedMoEMLP.quantize_fp8_).

    inplace=False works on a deep copy and leaves `model` as it is;
    inplace=True converts `model` itself and drops each bf16 weight as soon
    as its layer is converted, so peak memory stays near the bf16 model's.
    Returns the quantised model."""
    skip = (skip,) if isinstance(skip, str) else tuple(skip)
    if not inplace:
        model = copy.deepcopy(model)

    def make(name, lin):
        if any(name.endswith(s) for s in skip):
            return None
        new = ops.LinearW8.from_linear(lin)
        lin.weight = None  # the bf16 weight goes now, not with the old module
        lin.weight_t = None
        return new

    _swap(model, lambda m: isinstance(m, ops.Linear), make)
    for name, m in model.named_modules():
        if isinstance(m, FusedMoEMLP) \
                and not any(name.endswith(s) for s in skip):
            m.quantize_fp8_()
    return model


@torch.no_grad()
def dequantize_weights(model, dtype=None):
    """A copy of `model` in which every ops.LinearW8 is an ops.Linear whose
    weight is Wq = float(weight_q) * weight_scale[:, None], exactly, and
    every quantised FusedMoEMLP holds its represented matrices as parameters
    again. dtype
    defaults to that of the model's parameters (bf16 for a bf16 model, in
    which Wq is exact, as it is in fp32). `model` is not changed."""
    model = copy.deepcopy(model)
    if dtype is None:
        dtype = next((p.dtype for p in model.parameters()
                      if p.is_floating_point()), torch.bfloat16)

    def make(name, q):
        w = ops.dequantize_weight_fp8(q.weight_q, q.weight_scale, dtype)
        lin = ops.Linear(q.in_features, q.out_features, device="meta")
        lin.weight = torch.nn.Parameter(w)
        return lin

    _swap(model, lambda m: isinstance(m, ops.LinearW8), make)

    def make_moe(name, q):
        new = FusedMoEMLP(q.dim, q.intermediate, q.n_experts, q.top_k,
                          device="meta")
        new.router = q.router
        for w in ("w_gate_up", "w_down"):
            wq, scale = getattr(q, w), getattr(q, w + "_scale")
            full = torch.empty(wq.shape, dtype=dtype, device=wq.device)
            for e in range(wq.shape[0]):  # one expert's temporary at a time
                full[e] = ops.dequantize_weight_fp8(wq[e], scale[e], dtype)
            setattr(new, w, torch.nn.Parameter(full))
        return new

    _swap(model, lambda m: isinstance(m, FusedMoEMLP) and m.is_fp8, make_moe)
    return model
