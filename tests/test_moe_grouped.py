"""Fused MoE above 32 tokens: ops.moe_mlp through the gfx950 grouped GEMM
kernels (routing for any T, the counting sort into 64-row tiles, the gate/up
and down GEMMs over the tiles, the combine), bf16 and e4m3 expert weights.

Reference and bound are test_moe_fused's (float64, derived, independent of
the accumulation order); the e4m3 cases are test_moe_w8's, the reference
taken over the dequantised, exactly-bf16 matrices. Every test asserts
ops._moe_grouped_kernel_ok, so the composition cannot stand in for the
kernels; on a tree without them that assertion fails. Lines starting with
"[edges]" print measured error / bound; run with -s. Measured on MI355X:
worst error / bound 0.510 (bf16) and 0.809 (e4m3) in the accuracy cases, both
at E=3 k=1 D=128 I=128, 0.229 / 0.642 with one expert taking all and 0.434 at
the chunk boundary (profiles/moe_grouped.md).
"""
import pytest
import torch

import test_moe_fused as tmf
import test_moe_w8 as tw8
from kubetorch_amd import ops
from kubetorch_amd.models import FusedMoEMLP

pytestmark = pytest.mark.gpu
BM = ops.MOE_GROUPED_TILE_ROWS
WEIGHTS = ["bf16", "e4m3"]


def _args(wt, T, E, k, D, I):
    """CPU (x, logits, w_gate_up, w_down, scale_gate_up, scale_down) and the
    float64 (reference, bound); the scales are None for bf16 weights."""
    if wt == "e4m3":
        return tw8._case(T, E, k, D, I)
    args, rb = tmf._case(T, E, k, D, I)
    return (*args, None, None), rb


def _run(args, k):
    x, lg, wgu, wd, sgu, sd = (a if a is None else a.cuda() for a in args)
    assert ops._moe_grouped_kernel_ok(x, lg, wgu, wd, k, sgu, sd)
    return ops.moe_mlp(x, lg, wgu, wd, k, w_gate_up_scale=sgu, w_down_scale=sd)


@pytest.mark.parametrize("D,I", [(128, 128), (256, 384), (512, 256)])
@pytest.mark.parametrize("E,k", [(4, 2), (8, 8), (3, 1)])
@pytest.mark.parametrize("wt", WEIGHTS)
def test_accuracy_f64(wt, E, k, D, I):
    worst = 0.0
    for T in (33, BM - 1, BM, BM + 1, 2 * BM + 1):
        args, rb = _args(wt, T, E, k, D, I)
        out = _run(args, k)
        assert out.shape == (T, D) and out.dtype == torch.bfloat16
        worst = max(worst, tmf._ratio(out, rb))
    print(f"[edges] moe_mlp grouped {wt} E={E} k={k} D={D} I={I}: "
          f"error/bound {worst:.3f}")
    assert worst < 1.0, worst


@pytest.mark.parametrize("wt", WEIGHTS)
def test_one_expert_takes_all_and_idle_nan_weights_stay_out(wt):
    """Three tiles of one expert, the last with one row; the idle experts'
    weights (and scales) are NaN."""
    x, lg, wgu, wd, sgu, sd = _args(wt, 2 * BM + 1, 4, 1, 256, 384)[0]
    lg = lg.clone()
    lg[:, 2] = 10.0
    idle = [0, 1, 3]
    if wt == "e4m3":
        rb = tmf._ref_and_bound(x, lg, tw8._deq(wgu, sgu), tw8._deq(wd, sd), 1)
        wgu, wd = wgu.view(torch.uint8).clone(), wd.view(torch.uint8).clone()
        sgu, sd = sgu.clone(), sd.clone()
        wgu[idle], wd[idle] = 0x7F, 0x7F
        sgu[idle], sd[idle] = float("nan"), float("nan")
        wgu, wd = wgu.view(tw8.F8), wd.view(tw8.F8)
    else:
        rb = tmf._ref_and_bound(x, lg, wgu, wd, 1)
        wgu, wd = wgu.clone(), wd.clone()
        wgu[idle], wd[idle] = float("nan"), float("nan")
    out = _run((x, lg, wgu, wd, sgu, sd), 1)
    assert tmf._ratio(out, rb, f"grouped {wt} one expert") < 1


@pytest.mark.parametrize("wt", WEIGHTS)
def test_token_independence_and_determinism(wt):
    args, rb = _args(wt, 200, 8, 2, 256, 384)
    full = _run(args, 2)
    assert tmf._ratio(full, rb) < 1
    assert torch.equal(tmf._bits(_run(args, 2)), tmf._bits(full))
    head = _run((args[0][:33], args[1][:33], *args[2:]), 2)
    assert torch.equal(tmf._bits(head), tmf._bits(full[:33]))


@pytest.mark.parametrize("wt", WEIGHTS)
def test_strided_x(wt):
    B, S, D, E = 3, 15, 256, 4
    args, rb = _args(wt, B * S, E, 2, D, 384)
    wide = torch.full((B, S, 3 * D), float("nan"), dtype=torch.bfloat16,
                      device="cuda")
    wide[:, :, D:2 * D] = args[0].cuda().view(B, S, D)
    xs = wide[:, :, D:2 * D]
    assert xs.stride(1) == 3 * D and not xs.is_contiguous()
    out = _run((xs, args[1].view(B, S, E), *args[2:]), 2)
    assert out.shape == (B, S, D)
    assert torch.equal(tmf._bits(out.view(B * S, D)),
                       tmf._bits(_run(args, 2)))
    assert tmf._ratio(out.view(B * S, D), rb) < 1


def test_chunk_boundary():
    T = ops.MOE_GROUPED_MAX_ROWS + 1
    args, rb = _args("bf16", T, 4, 2, 128, 128)
    out = _run(args, 2)
    assert tmf._ratio(out, rb, f"grouped T={T}") < 1
    tail = _run((args[0][-33:], args[1][-33:], *args[2:]), 2)
    assert torch.equal(tmf._bits(tail[-1]), tmf._bits(out[-1]))


@pytest.mark.parametrize("wt", WEIGHTS)
def test_graph_capture_no_host_sync(wt):
    args, _ = _args(wt, 48, 8, 2, 256, 384)
    x, lg, wgu, wd, sgu, sd = (a if a is None else a.cuda() for a in args)
    assert ops._moe_grouped_kernel_ok(x, lg, wgu, wd, 2, sgu, sd)
    kw = dict(w_gate_up_scale=sgu, w_down_scale=sd)
    sx, sl = x.clone(), lg.clone()
    ops.moe_mlp(sx, sl, wgu, wd, 2, **kw)                 # warm up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.moe_mlp(sx, sl, wgu, wd, 2, **kw)
    for shift in (1, 5, 11):                              # new inputs
        nx, nl = x.roll(shift, 0), lg.roll(shift + 1, 0)
        want = ops.moe_mlp(nx, nl, wgu, wd, 2, **kw)
        sx.copy_(nx)
        sl.copy_(nl)
        graph.replay()
        assert torch.equal(tmf._bits(out), tmf._bits(want)), shift


def test_module_forward():
    torch.manual_seed(3)
    D = 256
    mod = FusedMoEMLP(D, 384, n_experts=4, top_k=2)
    with torch.no_grad():
        mod.w_gate_up.normal_(std=D ** -0.5)
        mod.w_down.normal_(std=384 ** -0.5)
    mod = mod.to("cuda", torch.bfloat16)
    x = torch.randn(2, 40, D, device="cuda", dtype=torch.bfloat16)
    for quantised in (False, True):
        if quantised:
            mod.quantize_fp8_()
        sc = dict(w_gate_up_scale=mod.w_gate_up_scale,
                  w_down_scale=mod.w_down_scale) if quantised else {}
        lg = mod.router(x)
        assert ops._moe_grouped_kernel_ok(x, lg, mod.w_gate_up, mod.w_down, 2,
                                          *sc.values())
        with torch.no_grad():
            out = mod(x)
            want = ops.moe_mlp(x, lg, mod.w_gate_up, mod.w_down, 2, **sc)
        assert out.shape == x.shape and bool(out.isfinite().all())
        assert torch.equal(tmf._bits(out), tmf._bits(want))
