"""Fused MoE decode: ops.moe_route, ops.moe_mlp (the gfx950 routed-GEMM
kernels and their torch composition), models.FusedMoEMLP / fuse_moe and the
serving engine's captured decode graph on a fused model.

The accuracy bound is derived, not tuned. With x and the weights as their
values in float64, h unrounded and w the float64 routing weights, per output

    |out - ref| <= 2^-8 |ref|                          output rounding
                 + sum_j w_j (dh_j @ |Wd_e|^T)         error of h
                 + I 2^-23 sum_j w_j (|h_j| @ |Wd_e|^T)  down accumulation
                 + 2^-20 |ref|                         fp32 routing weights
    dh = 2^-8 |h| + 2^-21 |h|
         + D 2^-23 (1.1 |u| (|x| @ |Wg|^T) + |silu(g)| (|x| @ |Wu|^T))

(h's rounding, fp32 exp, and the gate/up accumulation through SwiGLU's slope,
which is at most 1.1). Where the bound is 0 the result must be exact. Op
checks run on "cpu" (the composition) and on "cuda" under the gpu marker,
where _moe_kernel_ok is asserted so the kernel cannot silently be the
composition. Lines starting with "[edges]" print measured error / bound; run
with -s. Measured on MI355X: worst error / bound 0.355 (accuracy cases, at
E=3 k=1 D=128 I=128: the output-rounding term), 0.247 (one expert takes all)
and 0.129 (S = 1 and S = 2) through the kernels; 0.355 through the CPU
composition (profiles/moe_fused.md).
"""
import functools

import pytest
import torch

import test_paged_engine as tpe
from kubetorch_amd import ops
from kubetorch_amd.models import (BatchedGenerator, FusedMoEMLP, Llama,
                                  convert_to_moe, fuse_moe, llama_tiny)

BF16 = torch.bfloat16
RAISES = (RuntimeError, ValueError)
DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]


def _bits(t):
    return t.contiguous().view(torch.int16)


def _route64(logits, k):
    """Float64 routing of CPU logits: (sel [T, k], weights [T, k])."""
    v = logits.double()
    v = torch.where(v.isnan(), float("-inf"), v)
    vals, idx = torch.sort(v, dim=-1, descending=True, stable=True)
    vals = vals[:, :k]
    ex = torch.where(vals == vals[:, :1], 0.0, vals - vals[:, :1]).exp()
    return idx[:, :k], ex / ex.sum(-1, keepdim=True)


def _ref_and_bound(x, logits, wgu, wd, k):
    """Float64 reference of moe_mlp and the bound of the module docstring."""
    (E, D, I), T = wd.shape, x.shape[0]
    sel, w = _route64(logits, k)
    rows = torch.arange(T)[:, None]
    x, wd = x.double(), wd.double()
    wg, wu = wgu[:, :I].double(), wgu[:, I:].double()

    def up(a, m):     # [T, D] x [E, I, D] -> each pair's own expert [T, k, I]
        return torch.einsum("td,eid->tei", a, m)[rows, sel]

    def down(a, m):   # [T, k, I] -> [T, D], weighted over the k slots
        y = torch.einsum("tji,edi->tjed", a, m)
        return (y[rows, torch.arange(k)[None], sel] * w[..., None]).sum(1)

    g, u = up(x, wg), up(x, wu)
    silu = g * torch.sigmoid(g)
    h = silu * u
    ref = down(h, wd)
    dh = (2.0 ** -8 + 2.0 ** -21) * h.abs() + D * 2.0 ** -23 * (
        1.1 * u.abs() * up(x.abs(), wg.abs())
        + silu.abs() * up(x.abs(), wu.abs()))
    bound = (2.0 ** -8 + 2.0 ** -20) * ref.abs() + down(dh, wd.abs()) \
        + I * 2.0 ** -23 * down(h.abs(), wd.abs())
    return ref, bound


@functools.lru_cache(maxsize=None)
def _case(T, E, k, D, I, dtype=BF16):
    """CPU inputs (x, logits, w_gate_up, w_down) with their reference and
    bound; x's second row is zero, so its outputs have a zero bound."""
    gen = torch.Generator().manual_seed(T + 100 * E + 7 * k + D + 3 * I)
    x = torch.randn(T, D, generator=gen).to(dtype)
    x[1:2] = 0
    logits = (torch.randn(T, E, generator=gen) * 2).to(dtype)
    wgu = (torch.randn(E, 2 * I, D, generator=gen) * D ** -0.5).to(dtype)
    wd = (torch.randn(E, D, I, generator=gen) * I ** -0.5).to(dtype)
    return (x, logits, wgu, wd), _ref_and_bound(x, logits, wgu, wd, k)


def _run(device, args, k, kernel=True, **kw):
    args = [a.to(device) for a in args]
    if device == "cuda":
        assert ops._moe_kernel_ok(*args, k) == kernel
    return ops.moe_mlp(*args, k, **kw)


def _ratio(out, ref_bound, name=None):
    ref, bound = ref_bound
    err = (out.detach().cpu().double() - ref).abs()
    assert bool(out.isfinite().all())
    assert bool((err[bound == 0] == 0).all())
    ratio = float((err / bound.clamp_min(1e-300)).max())
    if name:
        print(f"[edges] moe_mlp {name}: error/bound {ratio:.3f}")
    return ratio


# ---------------------------------------------------------------------------
# Routing
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("E,k", [(3, 1), (3, 2), (8, 1), (8, 2), (8, 8),
                                 (64, 1), (64, 2), (64, 8)])
def test_route_matches_float64(device, E, k):
    gen = torch.Generator().manual_seed(E + k)
    lg = torch.randn(32, E, generator=gen) * 3           # distinct logits
    lg[8:16] = lg[8:16].round()                          # tie groups
    lg[16] = 0.5                                         # one tie group
    lg[17:20, ::2] = float("nan")
    lg[20:22, 1::3] = float("-inf")
    lg[22] = float("-inf")
    lg[23] = float("nan")
    lg[24] = torch.randperm(E, generator=gen) * 0.25     # distinct in bf16
    for dtype in (torch.float32, BF16):
        cast = lg.to(dtype)
        want_sel, want_w = _route64(cast, k)
        sel, w = ops.moe_route(cast.to(device), k)
        assert sel.dtype == torch.int32 and w.dtype == torch.float32
        assert torch.equal(sel.cpu().long(), want_sel)
        err = (w.cpu().double() - want_w).abs()
        assert bool((err <= 2.0 ** -22 * want_w).all()), float(
            (err / want_w.clamp_min(1e-300)).max())


# ---------------------------------------------------------------------------
# Accuracy against float64
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("D,I", [(128, 128), (256, 384), (512, 256)])
@pytest.mark.parametrize("E,k", [(4, 2), (8, 2), (3, 1), (8, 8)])
def test_accuracy_f64(device, E, k, D, I):
    worst = 0.0
    for T in (1, 3, 17, 32):
        args, rb = _case(T, E, k, D, I)
        # the float64 reference itself and the fp32 composition sit inside
        assert _ratio(ops.moe_mlp(*(a.double() for a in args), k), rb) < 1e-3
        out = _run(device, args, k)
        assert out.shape == (T, D) and out.dtype == BF16
        worst = max(worst, _ratio(out, rb))
    print(f"[edges] moe_mlp E={E} k={k} D={D} I={I} {device}: "
          f"error/bound {worst:.3f}")
    assert worst < 1.0, worst


# ---------------------------------------------------------------------------
# Sharp cases through the kernel
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_one_expert_takes_all_and_idle_nan_weights_stay_out_gpu():
    """32 rows in one expert's tile; the idle experts' weights are NaN."""
    (x, logits, wgu, wd), _ = _case(32, 4, 1, 256, 384)
    logits = logits.clone()
    logits[:, 2] = 10.0
    rb = _ref_and_bound(x, logits, wgu, wd, 1)
    idle = [0, 1, 3]
    wgu, wd = wgu.clone(), wd.clone()
    wgu[idle] = float("nan")
    wd[idle] = float("nan")
    assert _ratio(_run("cuda", (x, logits, wgu, wd), 1), rb, "one expert") < 1


@pytest.mark.gpu
def test_splits_and_determinism_gpu():
    E, k, D, I = 8, 2, 256, 1024
    args, rb = _case(17, E, k, D, I)
    S = ops.moe_down_splits(D, I, E, k)
    assert S > 1
    outs = {s: _run("cuda", args, k, num_splits=s) for s in (1, S, None)}
    assert _ratio(outs[1], rb, "S=1") < 1 and _ratio(outs[S], rb, f"S={S}") < 1
    assert torch.equal(_bits(outs[S]), _bits(outs[None]))
    assert torch.equal(_bits(outs[S]), _bits(_run("cuda", args, k)))


@pytest.mark.gpu
def test_token_alone_equals_token_in_batch_gpu():
    """The default S is the same at T = 1 and T = 32 (moe_down_splits does
    not depend on T), so a token's bits do not depend on its batch."""
    E, k, D, I = 8, 2, 256, 1024
    (x, logits, wgu, wd), rb = _case(32, E, k, D, I)
    assert ops.moe_down_splits(D, I, E, k) > 1
    dev = [a.cuda() for a in (x, logits, wgu, wd)]
    batch = ops.moe_mlp(*dev, k)
    assert _ratio(batch, rb) < 1
    for t in range(32):
        one = _run("cuda", (x[t:t + 1], logits[t:t + 1], dev[2], dev[3]), k)
        assert torch.equal(_bits(one[0]), _bits(batch[t])), t


@pytest.mark.gpu
def test_strided_x_gpu():
    (x, logits, wgu, wd), rb = _case(17, 4, 2, 256, 384)
    wide = torch.full((17, 3 * 256), float("nan"), dtype=BF16, device="cuda")
    wide[:, 256:512] = x.cuda()
    xs = wide[:, 256:512].view(17, 1, 256)        # a [B, 1, D] decode view
    assert xs.stride(0) == 768
    out = _run("cuda", (xs, logits.view(17, 1, 4), wgu, wd), 2)
    assert out.shape == (17, 1, 256)
    assert torch.equal(_bits(out.view(17, 256)),
                       _bits(_run("cuda", (x, logits, wgu, wd), 2)))
    assert _ratio(out.view(17, 256), rb) < 1


# ---------------------------------------------------------------------------
# Fallbacks and refusals
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("T,D,dtype", [(33, 256, BF16), (5, 256, torch.float32),
                                       (5, 192, BF16)])
def test_composition_serves_what_the_kernel_does_not(device, T, D, dtype):
    args, rb = _case(T, 4, 2, D, 128, dtype)
    out = _run(device, args, 2, kernel=False)
    assert out.dtype == dtype
    assert _ratio(out, rb, f"composition T={T} D={D} {dtype}") < 1


@pytest.mark.parametrize("device", DEVICES)
def test_refusals(device):
    (x, lg, wgu, wd), _ = _case(3, 4, 2, 128, 128)
    x, lg, wgu, wd = (a.to(device) for a in (x, lg, wgu, wd))
    ops.moe_mlp(x, lg, wgu, wd, 2)
    bad = [(x, lg, wgu, wd, 5),                       # top_k > E
           (x, lg, wgu, wd, 0),
           (x.float(), lg, wgu, wd, 2),               # mixed dtypes
           (x, lg.int(), wgu, wd, 2),
           (x, lg, wgu.to(torch.int32), wd.to(torch.int32), 2),
           (x[:, :64], lg, wgu, wd, 2),               # last dim is not D
           (x, lg[:, :3], wgu, wd, 2),                # logits are not [T, E]
           (x, lg[:2], wgu, wd, 2),
           (x, lg, wgu[:, :128], wd, 2),              # not [E, 2I, D]
           (x, lg, wgu[0], wd[0], 2),
           (x.to("meta"), lg, wgu, wd, 2)]            # devices
    if device == "cuda":
        bad += [(x.cpu(), lg, wgu, wd, 2), (x, lg.cpu(), wgu, wd, 2)]
    for call in bad:
        with pytest.raises(RAISES):
            ops.moe_mlp(*call)
    with pytest.raises(RAISES):
        ops.moe_mlp(x, lg, wgu, wd, 2, num_splits=65)
    with pytest.raises(RAISES):
        ops.moe_route(lg, 5)
    with pytest.raises(RuntimeError):                 # inference only
        ops.moe_mlp(x.clone().requires_grad_(True), lg, wgu, wd, 2)


# ---------------------------------------------------------------------------
# Model and engine
# ---------------------------------------------------------------------------
def _moe_model(**kw):
    torch.manual_seed(5)
    return convert_to_moe(Llama(llama_tiny(**kw)), n_experts=4, top_k=2).eval()


def test_fuse_moe_model_cpu():
    model = _moe_model().double()
    fused = fuse_moe(model)
    assert fused is not model and not hasattr(fused.layers[0].mlp, "ep_world")
    assert all(isinstance(ly.mlp, FusedMoEMLP) for ly in fused.layers)
    assert not any(isinstance(ly.mlp, FusedMoEMLP) for ly in model.layers)
    toks = torch.randint(0, model.cfg.vocab_size, (2, 24))
    with torch.no_grad():
        # both round the routing weights, MoEMLP also SwiGLU, through fp32
        torch.testing.assert_close(fused(toks), model(toks), rtol=1e-5,
                                   atol=1e-5)
    model.layers[1].mlp.ep_world = 2  # simulate an EP-sharded layer
    with pytest.raises(ValueError):
        fuse_moe(model)


@pytest.mark.parametrize("max_batch,want", [(32, True), (33, False)])
def test_engine_keeps_graph_up_to_32_rows(max_batch, want):
    eng = BatchedGenerator(fuse_moe(_moe_model()), max_batch=max_batch,
                           max_len=64, graph=True)
    assert eng._use_graph is want


@pytest.fixture(scope="module")
def gpu_fused():
    return fuse_moe(_moe_model(max_seq_len=192)).to("cuda", BF16)


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("kw", [dict(kv="slot"), dict(kv="paged", page_size=16),
                                dict(kv="paged", page_size=16,
                                     sampler="fused")],
                         ids=["slot", "paged", "paged-fused-sampler"])
def test_fused_decode_graph_matches_eager_gpu(gpu_fused, kw):
    prompts = tpe._gpu_prompts(gpu_fused.cfg)
    runs = {}
    for graph in (False, True):
        eng = BatchedGenerator(gpu_fused, max_batch=3, max_len=96, graph=graph,
                               **kw)
        rids = [eng.submit(p, max_new_tokens=12) for p in prompts[:2]]
        for _ in range(3):  # staggered join
            eng.step()
        rids += [eng.submit(p, max_new_tokens=12) for p in prompts[2:]]
        out = eng.run()
        runs[graph] = [out[r] for r in rids]
    assert eng._use_graph and len(eng._graphs) >= 1
    assert runs[True] == runs[False]
    for p, toks in zip(prompts, runs[True]):
        assert len(toks) == len(p) + 12
        tpe._assert_teacher_forced(gpu_fused, len(p), toks)
