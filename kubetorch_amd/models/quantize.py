"""FP8 weight-only quantisation of a model's ops.Linear layers.

quantize_weights_fp8 swaps every ops.Linear (wqkv, wo, w_gate_up, w_down,
lm_head of a Llama) for ops.LinearW8; the model's walk, generate() and
BatchedGenerator call the modules and run unchanged. dequantize_weights is
the way back: the same model with plain ops.Linear layers that hold the
matrix the fp8 layers represent, which is exactly representable in bf16.
"""
import copy

import torch

from kubetorch_amd import ops


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
    nn.Linear layers (MoE experts and router) are never touched.

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
    return model


@torch.no_grad()
def dequantize_weights(model, dtype=None):
    """A copy of `model` in which every ops.LinearW8 is an ops.Linear whose
    weight is Wq = float(weight_q) * weight_scale[:, None], exactly. dtype
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
    return model
