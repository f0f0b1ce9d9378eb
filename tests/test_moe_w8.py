"""FP8 expert weights for the fused MoE decode: ops.moe_mlp with e4m3
w_gate_up / w_down and per-row power-of-two scales (the W8A16 routed-GEMM
kernels and their composition), FusedMoEMLP under models.quantize_weights_fp8
/ dequantize_weights, and the engine's decode graph on the quantised model.

The reference and the bound are test_moe_fused's, verbatim, with the
represented matrices float(q) * scale[..., None] passed in as the weights:
they are exactly bf16, so the only errors are the ones that bound counts.
Every op test here raises ValueError without the feature. Lines starting with
"[edges]" print measured error / bound; run with -s. Measured on MI355X
through the kernels: worst error / bound 0.672 (accuracy cases, at E=8 k=8
D=128 I=128), 0.490 (code points, gate; 0.327 up and down), 0.382 (S = 1) and
0.475 (idle experts); 0.672 through the CPU composition too
(profiles/moe_w8.md).
"""
import functools

import pytest
import torch

import test_paged_engine as tpe
from kubetorch_amd import ops
from kubetorch_amd.models import (BatchedGenerator, FusedMoEMLP, MoEMLP,
                                  dequantize_weights, fuse_moe,
                                  quantize_weights_fp8)
from test_moe_fused import DEVICES, _bits, _moe_model, _ratio, _ref_and_bound

BF16 = torch.bfloat16
F8 = torch.float8_e4m3fn
RAISES = (RuntimeError, ValueError)


def _quant(w):
    """[E, N, K] float -> (e4m3 [E, N, K], fp32 scales [E, N]), per expert."""
    qs = [ops.quantize_weight_fp8(m) for m in w]
    return (torch.stack([q.view(torch.uint8) for q, _ in qs]).view(F8),
            torch.stack([s for _, s in qs]))


def _deq(q, s):
    return q.float() * s[..., None]


@functools.lru_cache(maxsize=None)
def _case(T, E, k, D, I):
    """CPU inputs (x, logits, q_gate_up, q_down, s_gate_up, s_down) with the
    float64 reference and bound of the represented matrices. Every weight row
    is multiplied by a seeded power of two in [2^-6, 2^3] before quantising,
    so a scale of the wrong row, expert or half is a large error. x's second
    row is zero: a zero bound."""
    gen = torch.Generator().manual_seed(T + 100 * E + 7 * k + D + 3 * I)
    x = torch.randn(T, D, generator=gen).to(BF16)
    x[1:2] = 0
    logits = (torch.randn(T, E, generator=gen) * 2).to(BF16)

    def weight(n, kdim):
        p = torch.randint(-6, 4, (E, n, 1), generator=gen).float()
        return torch.randn(E, n, kdim, generator=gen) * kdim ** -0.5 * 2.0 ** p

    (qgu, sgu), (qd, sd) = _quant(weight(2 * I, D)), _quant(weight(D, I))
    return (x, logits, qgu, qd, sgu, sd), _ref_and_bound(
        x, logits, _deq(qgu, sgu), _deq(qd, sd), k)


def _run(device, args, k, **kw):
    x, lg, qgu, qd, sgu, sd = (a.to(device) for a in args)
    if device == "cuda":
        assert ops._moe_kernel_ok(x, lg, qgu, qd, k, sgu, sd)
    return ops.moe_mlp(x, lg, qgu, qd, k, w_gate_up_scale=sgu,
                       w_down_scale=sd, **kw)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("D,I", [(128, 128), (256, 384), (512, 256)])
@pytest.mark.parametrize("E,k", [(3, 1), (8, 2), (8, 8)])
def test_accuracy_f64(device, E, k, D, I):
    worst = 0.0
    for T in (1, 3, 17, 32):
        args, rb = _case(T, E, k, D, I)
        # the float64 composition on the same bytes is the reference itself
        assert _ratio(_run("cpu", [args[0].double(), *args[1:]], k), rb) < 1e-3
        out = _run(device, args, k)
        assert out.shape == (T, D) and out.dtype == BF16
        worst = max(worst, _ratio(out, rb))
    print(f"[edges] moe_mlp w8 E={E} k={k} D={D} I={I} {device}: "
          f"error/bound {worst:.3f}")
    assert worst < 1.0, worst


POSITIONS = (0, 7, 8, 15, 16, 31, 32, 127, 128, 255)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("which", ["up", "down", "gate"])
def test_code_points_and_k_permutation(device, which):
    """Row t of x is one-hot at POSITIONS[t] and the other two matrices are
    identities or ones, so every output element is one entry of the matrix
    under test (times silu(1) or through silu): all 254 non-NaN codes in
    every column, a distinct scale per row."""
    E, D = 2, 256
    codes = torch.tensor([b for b in range(256) if b & 0x7F != 0x7F],
                         dtype=torch.uint8)
    n, col = torch.arange(D)[:, None], torch.arange(D)[None]
    under = codes[(n + 7 * col) % 254].view(F8)
    cyc = 2.0 ** (torch.arange(D) % 16 - 12).float()
    eye = torch.eye(D).to(F8)                       # byte 0x38 on the diagonal
    ones, unit = torch.ones(D, D).to(F8), torch.ones(D)
    gate, up, down = (ones, unit), (eye if which == "down" else ones, unit), \
        (eye, unit)
    if which == "gate":
        gate = (under, torch.full((D,), 2.0 ** -6))  # |g| <= 7
    elif which == "up":
        up = (under, cyc)
    else:
        down = (under, cyc)
    qgu = torch.cat([gate[0].view(torch.uint8), up[0].view(torch.uint8)])
    qgu = qgu.expand(E, 2 * D, D).contiguous().view(F8)
    qd = down[0].view(torch.uint8).expand(E, D, D).contiguous().view(F8)
    sgu = torch.cat([gate[1], up[1]]).expand(E, 2 * D).contiguous()
    sd = down[1].expand(E, D).contiguous()
    x = torch.zeros(len(POSITIONS), D, dtype=BF16)
    x[torch.arange(len(POSITIONS)), list(POSITIONS)] = 1
    logits = torch.randn(len(POSITIONS), E,
                         generator=torch.Generator().manual_seed(3)).to(BF16)
    rb = _ref_and_bound(x, logits, _deq(qgu, sgu), _deq(qd, sd), 1)
    out = _run(device, (x, logits, qgu, qd, sgu, sd), 1)
    assert _ratio(out, rb, f"w8 codes {which} {device}") < 1


@pytest.mark.gpu
def test_bits_gpu():
    E, k, D, I = 8, 2, 256, 1024
    args, rb = _case(32, E, k, D, I)
    S = ops.moe_down_splits(D, I, E, k)
    assert S > 1
    batch = _run("cuda", args, k)
    assert _ratio(batch, rb) < 1
    assert torch.equal(_bits(_run("cuda", args, k, num_splits=S)), _bits(batch))
    assert torch.equal(_bits(_run("cuda", args, k)), _bits(batch))
    assert _ratio(_run("cuda", args, k, num_splits=1), rb, "w8 S=1") < 1
    dev = [a.cuda() for a in args]
    for t in range(32):                              # a token alone
        one = _run("cuda", (dev[0][t:t + 1], dev[1][t:t + 1], *dev[2:]), k)
        assert torch.equal(_bits(one[0]), _bits(batch[t])), t
    wide = torch.full((32, 3 * D), float("nan"), dtype=BF16, device="cuda")
    wide[:, D:2 * D] = dev[0]
    xs = wide[:, D:2 * D].view(32, 1, D)             # a [T, 1, D] decode view
    assert xs.stride(0) == 3 * D
    out = _run("cuda", (xs, dev[1].view(32, 1, E), *dev[2:]), k)
    assert torch.equal(_bits(out.view(32, D)), _bits(batch))


@pytest.mark.gpu
def test_idle_experts_nan_bytes_stay_out_gpu():
    x, logits, qgu, qd, sgu, sd = _case(32, 4, 1, 256, 384)[0]
    logits = logits.clone()
    logits[:, 2] = 10.0
    rb = _ref_and_bound(x, logits, _deq(qgu, sgu), _deq(qd, sd), 1)
    idle = [0, 1, 3]
    qgu, qd = qgu.view(torch.uint8).clone(), qd.view(torch.uint8).clone()
    sgu, sd = sgu.clone(), sd.clone()
    qgu[idle], qd[idle] = 0x7F, 0x7F
    sgu[idle], sd[idle] = 2.0 ** 40, 2.0 ** 40
    out = _run("cuda", (x, logits, qgu.view(F8), qd.view(F8), sgu, sd), 1)
    assert _ratio(out, rb, "w8 idle experts") < 1


@pytest.mark.parametrize("device", DEVICES)
def test_refusals(device):
    x, lg, qgu, qd, sgu, sd = (a.to(device) for a in _case(3, 3, 1, 128, 128)[0])
    wgu, wd = _deq(qgu, sgu).to(BF16), _deq(qd, sd).to(BF16)
    other = "cpu" if device == "cuda" else "meta"
    bad = [(wgu, qd, sgu, sd), (qgu, wd, sgu, sd),      # one fp8, one bf16
           (wgu, qd, None, None),
           (qgu.to(torch.float8_e5m2), qd.to(torch.float8_e5m2), sgu, sd),
           (qgu.to(torch.float8_e4m3fnuz), qd.to(torch.float8_e4m3fnuz),
            sgu, sd),
           (wgu, wd, sgu, sd), (wgu, wd, sgu, None),    # scales with bf16
           (qgu, qd, None, None), (qgu, qd, sgu, None), (qgu, qd, None, sd),
           (qgu, qd, sgu[:, :-1], sd), (qgu, qd, sgu, sd[0]),
           (qgu, qd, sd, sgu), (qgu, qd, sgu.double(), sd),
           (qgu, qd, sgu, sd.to(BF16)), (qgu, qd, sgu.to(other), sd),
           (qgu, qd, sgu, sd.to(other))]
    if device == "cpu":
        bad += [(qgu, qd, sgu * 1.5, sd), (qgu, qd, sgu, sd * 0),
                (qgu, qd, sgu, sd * 2.0 ** 60)]
    for a, b, c, d in bad:
        with pytest.raises(ValueError):
            ops.moe_mlp(x, lg, a, b, 1, w_gate_up_scale=c, w_down_scale=d)
    with pytest.raises(RAISES):                          # x is not a float
        ops.moe_mlp(x.int(), lg, qgu, qd, 1, w_gate_up_scale=sgu,
                    w_down_scale=sd)
    with pytest.raises(RAISES):
        ops.moe_mlp(x, lg, qgu, qd, 1, num_splits=65, w_gate_up_scale=sgu,
                    w_down_scale=sd)
    with pytest.raises(RuntimeError):                    # inference only
        ops.moe_mlp(x.clone().requires_grad_(True), lg, qgu, qd, 1,
                    w_gate_up_scale=sgu, w_down_scale=sd)


def test_quantised_fused_model_cpu():
    base = _moe_model()
    model = quantize_weights_fp8(fuse_moe(base))
    for ly in model.layers:
        m, bufs = ly.mlp, dict(ly.mlp.named_buffers(recurse=False))
        assert isinstance(m, FusedMoEMLP) and "weight=e4m3" in repr(m)
        assert sorted(bufs) == ["w_down", "w_down_scale", "w_gate_up",
                                "w_gate_up_scale"]
        assert [n for n, _ in m.named_parameters()] == ["router.weight"]
        assert m.w_gate_up.dtype == m.w_down.dtype == F8
        assert m.w_gate_up_scale.dtype == m.w_down_scale.dtype == torch.float32
        assert m.w_gate_up_scale.shape == m.w_gate_up.shape[:2]
        assert m.w_down_scale.shape == m.w_down.shape[:2]
    unfused = quantize_weights_fp8(base)                 # experts left alone
    assert all(isinstance(ly.mlp, MoEMLP) and all(
        type(ex.w_down) is torch.nn.Linear for ex in ly.mlp.experts)
        for ly in unfused.layers)
    sd = model.state_dict()
    torch.manual_seed(11)
    fresh = quantize_weights_fp8(fuse_moe(_moe_model()))
    for p in fresh.layers[0].mlp.buffers():
        p.view(torch.uint8).zero_()
    fresh.load_state_dict(sd)
    cast = fresh.to(BF16)
    for (n, a), (_, b) in zip(sd.items(), cast.state_dict().items()):
        if "mlp.w_" in n:
            assert a.dtype == b.dtype
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), n
    deq = dequantize_weights(model)
    for q, d in zip(model.layers, deq.layers):
        assert isinstance(d.mlp, FusedMoEMLP) and not d.mlp.is_fp8
        for n in ("w_gate_up", "w_down"):
            w = getattr(d.mlp, n)
            assert isinstance(w, torch.nn.Parameter)
            assert torch.equal(w.float(), _deq(getattr(q.mlp, n),
                                               getattr(q.mlp, n + "_scale")))
    toks = torch.randint(0, model.cfg.vocab_size, (2, 24))
    with torch.no_grad():
        torch.testing.assert_close(model.double()(toks), deq.double()(toks),
                                   rtol=1e-9, atol=1e-9)


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_quantised_decode_graph_matches_eager_gpu():
    model = quantize_weights_fp8(
        fuse_moe(_moe_model(max_seq_len=192)).to("cuda", BF16), inplace=True)
    prompts = tpe._gpu_prompts(model.cfg)
    runs = {}
    for graph in (False, True):
        eng = BatchedGenerator(model, max_batch=3, max_len=96, graph=graph,
                               kv="paged", page_size=16)
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
        tpe._assert_teacher_forced(model, len(p), toks)
