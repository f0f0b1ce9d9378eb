"""attn_grad_pack (GQA group sum + RoPE^T + qkv packing in one kernel) and
the ops.qkv_attention autograd node built on it.

Error bound of the pack kernel, per output element, against the same
formula in float64 computed from the bf16 inputs:

    |out - ref| <= 2^-8 * |ref| + (g + 3) * 2^-24 * A

bf16 keeps 8 significant bits, so its one round-to-nearest is at most 2^-8
relative. The fp32 part: the inputs are exact in fp32; a group sum of g
terms takes g - 1 roundings, each at most 2^-24 of a partial sum that is
itself at most the sum of absolute values; the two products and their sum
add 2 more and the scale 1, so g + 2 in all, and g + 3 covers the second-
order terms and the 2^-8 the final rounding puts on the fp32 error. A is
the sum of absolute values of the terms that enter the element:
sum_j |dv_e_j| for v, and q_oscale * (|c| * sum_j |a_j| + |s| * sum_j |b_j|)
for the rotated parts (a, b the two halves of the head dim, one j for q).

The separate sum / rope / cat composition rounds the group sums to bf16
before the rotation. That first rounding is at most 2^-8 of |a| and |b|,
so 2^-8 * A on the element, on which the second rounding puts a further
2^-8: its bound is 2^-8 * |ref| + ((1 + 2^-6) * 2^-8 + (g + 3) * 2^-24) * A.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from kubetorch_amd import ops
from kubetorch_amd.models import Llama, LlamaConfig

BF16 = torch.bfloat16

# (B, Hq, Hkv, S, D)
SHAPES = [
    (2, 2, 2, 3, 8),          # g=1, smallest D, odd S, fewer items than a block
    (2, 4, 1, 17, 64),        # g=4
    (1, 8, 1, 5, 128),        # g=8
    (2, 8, 2, 256, 128),      # the model's ratio
    (2, 32, 8, 1024, 128),    # more items than one pass of the capped grid
]
OSCALES = [1.0, 128 ** -0.5 * ops.LOG2E]
LAYOUTS = ["bhsd", "bshd", "mixed"]


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    """Seeded bf16 (dq, dk_e, dv_e) on the CPU and position-dependent fp32
    tables; never modified."""
    B, Hq, Hkv, S, D = shape
    gen = torch.Generator().manual_seed(1000 + sum(shape))
    dq, dk, dv = (torch.randn(B, Hq, S, D, generator=gen).to(BF16)
                  for _ in range(3))
    cos, sin = ops.precompute_rope(S + 3, D)   # a table longer than S
    return dq, dk, dv, cos, sin


@functools.lru_cache(maxsize=None)
def _ref64(shape, oscale):
    """(ref, A) in float64, both [B, S, (Hq + 2*Hkv)*D]."""
    B, Hq, Hkv, S, D = shape
    g = Hq // Hkv
    dq, dk, dv, cos, sin = _inputs(shape)
    c = cos[:S].double().view(1, 1, S, D // 2)
    s = sin[:S].double().view(1, 1, S, D // 2)

    def group(x):          # -> (sum_j x_j, sum_j |x_j|), [B, Hkv, S, D]
        x = x.double().view(B, Hkv, g, S, D)
        return x.sum(2), x.abs().sum(2)

    def rot_t(x, xabs, osc):
        a, b = x[..., :D // 2], x[..., D // 2:]
        aa, ab = xabs[..., :D // 2], xabs[..., D // 2:]
        ref = torch.cat([a * c + b * s, b * c - a * s], -1) * osc
        amp = torch.cat([aa * c.abs() + ab * s.abs(),
                         ab * c.abs() + aa * s.abs()], -1) * osc
        return ref, amp

    qr, qa = rot_t(dq.double(), dq.double().abs(), oscale)
    kr, ka = rot_t(*group(dk), 1.0)
    vr, va = group(dv)

    def pack(q, k, v):
        return torch.cat([t.transpose(1, 2).reshape(B, S, -1)
                          for t in (q, k, v)], -1)

    return pack(qr, kr, vr), pack(qa, ka, va)


def _bound(shape, oscale, two_roundings):
    g = shape[1] // shape[2]
    ref, amp = _ref64(shape, oscale)
    first = (1 + 2.0 ** -6) * 2.0 ** -8 if two_roundings else 0.0
    return 2.0 ** -8 * ref.abs() + (first + (g + 3) * 2.0 ** -24) * amp


def _assert_within(out, shape, oscale, two_roundings):
    ref, _ = _ref64(shape, oscale)
    assert out.shape == ref.shape and out.dtype == BF16
    err = (out.double().cpu() - ref).abs()
    bound = _bound(shape, oscale, two_roundings)
    ratio = (err / bound.clamp(min=1e-300)).max().item()
    print(f"{shape} oscale={oscale:.4f} two_roundings={two_roundings}: "
          f"max err/bound {ratio:.3f}, max err {err.max().item():.3e}")
    bad = err > bound          # every element, none left out
    assert not bad.any(), (
        f"{int(bad.sum())} of {bad.numel()} elements over the bound, "
        f"worst err/bound {ratio:.3f}")


def _layout(t, kind):
    """The same values as a [B,H,S,D] buffer or as a transposed view of a
    [B,S,H,D] buffer."""
    if kind == "bshd":
        v = t.transpose(1, 2).contiguous().transpose(1, 2)
        assert v.stride(1) == t.shape[3] or t.shape[1] == 1
        return v
    return t.contiguous()


def _on(device, shape, layout):
    dq, dk, dv, cos, sin = _inputs(shape)
    kinds = {"bhsd": ("bhsd",) * 3, "bshd": ("bshd",) * 3,
             "mixed": ("bshd", "bhsd", "bshd")}[layout]
    dq, dk, dv = (_layout(t.to(device), k)
                  for t, k in zip((dq, dk, dv), kinds))
    return dq, dk, dv, cos.to(device), sin.to(device)


class _NoPackKernel:
    """Stands in for the extension; an attn_grad_pack launch is an error."""

    def __init__(self, ext):
        self._ext = ext

    def __getattr__(self, name):
        if name == "attn_grad_pack":
            raise AssertionError("attn_grad_pack kernel launched")
        return getattr(self._ext, name)


class _CountPackKernel:
    """Passes through to the extension and counts attn_grad_pack calls."""

    def __init__(self, ext):
        self._ext = ext
        self.calls = 0
        self.names = set()      # every extension function asked for

    def __getattr__(self, name):
        self.names.add(name)
        if name == "attn_grad_pack":
            self.calls += 1
        return getattr(self._ext, name)


# ---------------------------------------------------------------------------
# (a) the pack against fp64
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("oscale", OSCALES, ids=["one", "v3scale"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_pack_reference_composition_cpu(shape, oscale):
    """Off the GPU attn_grad_pack is the sum / rope / cat composition; it
    meets the two-rounding bound, which shows the fp64 reference is wired
    the way the code it replaces is."""
    dq, dk, dv, cos, sin = _on("cpu", shape, "bhsd")
    out = ops.attn_grad_pack(dq, dk, dv, cos, sin, shape[2], oscale)
    _assert_within(out, shape, oscale, two_roundings=True)


@pytest.mark.gpu
@pytest.mark.parametrize("oscale", OSCALES, ids=["one", "v3scale"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_pack_kernel_gpu(shape, layout, oscale, monkeypatch):
    dq, dk, dv, cos, sin = _on("cuda", shape, layout)
    proxy = _CountPackKernel(ops._ext())
    monkeypatch.setattr(ops, "_ext", lambda: proxy)
    out = ops.attn_grad_pack(dq, dk, dv, cos, sin, shape[2], oscale)
    assert proxy.calls == 1, "the kernel must take both layouts without a copy"
    assert out.is_contiguous()
    _assert_within(out, shape, oscale, two_roundings=False)


@pytest.mark.gpu
@pytest.mark.parametrize("oscale", OSCALES, ids=["one", "v3scale"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_pack_reference_composition_gpu(shape, oscale):
    dq, dk, dv, cos, sin = _on("cuda", shape, "bshd")
    out = ops._attn_grad_pack_ref(dq, dk, dv, cos[:shape[3]], sin[:shape[3]],
                                  shape[2], oscale)
    _assert_within(out, shape, oscale, two_roundings=True)


# ---------------------------------------------------------------------------
# (b) argument checks: the binding raises, the wrapper falls back, and
# neither launches
# ---------------------------------------------------------------------------
def _bad_layouts(device):
    """name -> (dq, dk_e, dv_e) with one tensor the kernel cannot take."""
    B, Hq, S, D = 2, 4, 6, 16
    gen = torch.Generator().manual_seed(11)

    def rnd(*shape):
        return torch.randn(*shape, generator=gen).to(BF16).to(device)

    good = [rnd(B, Hq, S, D) for _ in range(3)]
    cases = {}
    cases["stride3"] = [rnd(B, Hq, S, 2 * D)[..., ::2]] + good[1:]
    cases["token_stride"] = [good[0], rnd(B, Hq, S, D + 4)[..., :D], good[2]]
    cases["base_pointer"] = good[:2] + [rnd(B, Hq, S, D + 8)[..., 4:D + 4]]
    for name, (a, b, c) in cases.items():
        assert a.shape == b.shape == c.shape == (B, Hq, S, D), name
    return cases, ops.precompute_rope(S, D, device=device)


def _check_fallback(device, monkeypatch):
    cases, (cos, sin) = _bad_layouts(device)
    if device == "cuda":
        proxy = _NoPackKernel(ops._ext())
        monkeypatch.setattr(ops, "_ext", lambda: proxy)
    for name, (dq, dk, dv) in cases.items():
        out = ops.attn_grad_pack(dq, dk, dv, cos, sin, 2, 0.5)
        want = ops._attn_grad_pack_ref(dq, dk, dv, cos, sin, 2, 0.5)
        assert torch.equal(out.view(torch.int16), want.view(torch.int16)), name
    dq, dk, dv = (t.contiguous() for t in cases["stride3"])
    with pytest.raises(ValueError):
        ops.attn_grad_pack(dq, dk[:, :2], dv, cos, sin, 2, 1.0)
    with pytest.raises(ValueError):
        ops.attn_grad_pack(dq, dk, dv, cos, sin, 3, 1.0)     # Hq=4 % 3
    with pytest.raises(ValueError):
        ops.attn_grad_pack(dq, dk, dv, cos[:4], sin[:4], 2, 1.0)   # S=6 rows


def test_pack_wrapper_falls_back_cpu(monkeypatch):
    _check_fallback("cpu", monkeypatch)


@pytest.mark.gpu
def test_pack_wrapper_falls_back_gpu(monkeypatch):
    _check_fallback("cuda", monkeypatch)


@pytest.mark.gpu
def test_pack_binding_raises():
    ext = ops._ext()
    cases, (cos, sin) = _bad_layouts("cuda")
    for name, (dq, dk, dv) in cases.items():
        with pytest.raises(RuntimeError):
            ext.attn_grad_pack(dq, dk, dv, cos, sin, 2, 1.0)
    dq, dk, dv = (t.contiguous() for t in cases["stride3"])
    bad_calls = {
        "shape": (dq, dk[:, :2], dv, cos, sin, 2),
        "groups": (dq, dk, dv, cos, sin, 3),
        "n_kv": (dq, dk, dv, cos, sin, 0),
        "table_rows": (dq, dk, dv, cos[:4], sin[:4], 2),
        "table_dtype": (dq, dk, dv, cos.double(), sin.double(), 2),
        "table_device": (dq, dk, dv, cos.cpu(), sin.cpu(), 2),
        "dtype": (dq.float(), dk.float(), dv.float(), cos, sin, 2),
        "cpu": (dq.cpu(), dk.cpu(), dv.cpu(), cos, sin, 2),
    }
    for name, args in bad_calls.items():
        with pytest.raises(RuntimeError):
            ext.attn_grad_pack(*args, 1.0)
    torch.cuda.synchronize()
    # and the same tensors are accepted once nothing is wrong with them
    ext.attn_grad_pack(dq, dk, dv, cos, sin, 2, 1.0)


# ---------------------------------------------------------------------------
# (c) the node
# ---------------------------------------------------------------------------
def _rope_t64(x, cos, sin, osc):
    """oscale * R^T(x) in float64, x [B, H, S, D]."""
    D = x.shape[-1]
    S = x.shape[2]
    c = cos[:S].double().view(1, 1, S, D // 2)
    s = sin[:S].double().view(1, 1, S, D // 2)
    a, b = x.double()[..., :D // 2], x.double()[..., D // 2:]
    return torch.cat([a * c + b * s, b * c - a * s], -1) * osc


def _separate_nodes(qkv, gout, cos, sin, Hq, Hkv, impl):
    """The composition the node replaces, written out from ops.rope and
    ops.flash_attention alone (no helper of the node): split views, rope
    nodes, the flash_attention node, and autograd's own sum / rope backward
    / cat. -> (o, dqkv, rotated q, rotated k, v, scale folded into q)."""
    B, S, W = qkv.shape
    D = W // (Hq + 2 * Hkv)
    x = qkv.clone().requires_grad_(True)
    q, k, v = x.split([Hq * D, Hkv * D, Hkv * D], dim=-1)
    osc = D ** -0.5 * math.log2(math.e) if impl == "v3" else 1.0
    q = ops.rope(q.view(B, S, Hq, D), cos, sin, oscale=osc).transpose(1, 2)
    k = ops.rope(k.view(B, S, Hkv, D), cos, sin).transpose(1, 2)
    v = v.view(B, S, Hkv, D).transpose(1, 2)
    o = ops.flash_attention(q, k, v, impl=impl)
    o = o.transpose(1, 2).reshape(B, S, -1)
    o.backward(gout)
    return o.detach(), x.grad, q.detach(), k.detach(), v.detach(), osc


@pytest.mark.gpu
@pytest.mark.parametrize("bwd", ["aten", "ckbwd"])
@pytest.mark.parametrize("grad_layout", ["strided", "contiguous"])
@pytest.mark.parametrize("impl", ["v3", "ck"])
def test_qkv_attention_node_gpu(impl, grad_layout, bwd, monkeypatch):
    """grad_layout "strided" is the node as the model runs it: grad_out
    reaches the dense backward as the [B,H,S,D] view of the [B,S,H*D]
    gradient. "contiguous" is the node's backward with a [B,H,S,D]-contiguous
    grad_out, which the node itself never makes, so its three steps are
    called in the node's order. bwd "ckbwd" sets KT_ATTN_BWD=ck, whose
    dq/dk_e/dv_e go straight into the pack kernel."""
    B, Hq, Hkv, S, D = 2, 8, 2, 256, 128
    g = Hq // Hkv
    torch.manual_seed(3)
    qkv = torch.randn(B, S, (Hq + 2 * Hkv) * D, dtype=BF16, device="cuda")
    gout = torch.randn(B, S, Hq * D, dtype=BF16, device="cuda")
    cos, sin = ops.precompute_rope(S, D, device="cuda")
    if bwd == "ckbwd":
        monkeypatch.setenv("KT_ATTN_BWD", "ck")
    else:
        monkeypatch.delenv("KT_ATTN_BWD", raising=False)

    o0, g0, q, k, v, osc = _separate_nodes(qkv, gout, cos, sin, Hq, Hkv, impl)
    assert o0.shape == (B, S, Hq * D) and g0.shape == qkv.shape
    sm_scale = math.log(2.0) if impl == "v3" else D ** -0.5

    monkeypatch.setenv("KT_ATTN_PACK", "1")
    proxy = _CountPackKernel(ops._ext())
    monkeypatch.setattr(ops, "_ext", lambda: proxy)
    if grad_layout == "strided":
        x1 = qkv.clone().requires_grad_(True)
        o1 = ops.qkv_attention(x1, cos, sin, Hq, Hkv, impl)
        o1.backward(gout)
        g1 = x1.grad
    else:
        qs, ks, vs, o_bhsd, lse, scale = ops._attention_forward(
            q, k, v, D ** -0.5, impl)
        assert scale == pytest.approx(sm_scale, rel=1e-12)
        o1 = o_bhsd.transpose(1, 2).reshape(B, S, -1)
        go = gout.view(B, S, Hq, D).transpose(1, 2).contiguous()
        g1 = ops.attn_grad_pack(
            *ops._attention_backward_expanded(go, qs, ks, vs, o_bhsd, lse,
                                              scale),
            cos, sin, Hkv, osc)
    assert proxy.calls == 1
    assert ("attn_bwd_ck" in proxy.names) == (bwd == "ckbwd")

    # forward: the same kernels as the separate nodes, so the same bits
    assert o1.shape == o0.shape and g1.shape == qkv.shape
    assert torch.equal(o1.view(torch.int16), o0.view(torch.int16))

    # backward: fp32 SDPA on the rotated bf16 q/k the kernels saw, built as
    # in tests/test_ops.py::test_v3_prescaled_fwd_bwd, then the exact
    # (float64) rotation back and the packing
    qr, kr, vr = (t.float().requires_grad_(True) for t in (q, k, v))
    outr = F.scaled_dot_product_attention(
        qr, kr.repeat_interleave(g, 1), vr.repeat_interleave(g, 1),
        is_causal=True, scale=sm_scale)
    outr.backward(gout.view(B, S, Hq, D).transpose(1, 2).float())
    parts = {
        "q": (_rope_t64(qr.grad, cos, sin, osc), 0, Hq * D),
        "k": (_rope_t64(kr.grad, cos, sin, 1.0), Hq * D, Hkv * D),
        "v": (vr.grad.double(), (Hq + Hkv) * D, Hkv * D),
    }
    for name, (ref, start, width) in parts.items():
        ref = ref.transpose(1, 2).reshape(B, S, width).float()
        atol = max(2e-2, 6e-3 * ref.abs().max().item())
        for tag, got in (("pack", g1), ("separate", g0)):
            got = got[..., start:start + width].float()
            print(f"{impl} {grad_layout} {bwd} d{name} {tag}: max err "
                  f"{(got - ref).abs().max().item():.4f}, atol {atol:.4f}")
            torch.testing.assert_close(got, ref, rtol=2e-2, atol=atol,
                                       msg=f"{impl} d{name} ({tag})")


def test_qkv_attention_composition_cpu(monkeypatch):
    """Off the GPU both settings of the switch run the separate nodes, with
    SDPA in place of the forward kernel."""
    B, Hq, Hkv, S, D = 2, 4, 2, 9, 16
    torch.manual_seed(5)
    qkv = torch.randn(B, S, (Hq + 2 * Hkv) * D)
    cos, sin = ops.precompute_rope(S, D)
    gout = torch.randn(B, S, Hq * D)

    def manual(impl):
        x = qkv.clone().requires_grad_(True)
        q, k, v = x.split([Hq * D, Hkv * D, Hkv * D], dim=-1)
        osc = D ** -0.5 * ops.LOG2E if impl == "v3" else 1.0
        q = ops.rope(q.view(B, S, Hq, D), cos, sin, oscale=osc).transpose(1, 2)
        k = ops.rope(k.view(B, S, Hkv, D), cos, sin).transpose(1, 2)
        v = v.view(B, S, Hkv, D).transpose(1, 2)
        o = F.scaled_dot_product_attention(
            q, k.repeat_interleave(2, 1), v.repeat_interleave(2, 1),
            is_causal=True, scale=ops._LN2 if impl == "v3" else D ** -0.5)
        o = o.transpose(1, 2).reshape(B, S, -1)
        o.backward(gout)
        return o.detach(), x.grad

    for impl in ("v3", "ck"):
        want_o, want_g = manual(impl)
        for switch in ("0", "1"):
            monkeypatch.setenv("KT_ATTN_PACK", switch)
            x = qkv.clone().requires_grad_(True)
            o = ops.qkv_attention(x, cos, sin, Hq, Hkv, impl)
            o.backward(gout)
            assert torch.equal(o, want_o) and torch.equal(x.grad, want_g)
    # the same attention whichever way the scale reaches the scores
    torch.testing.assert_close(manual("v3")[0], manual("ck")[0],
                               rtol=1e-4, atol=1e-5)
    with pytest.raises(ValueError):
        ops.qkv_attention(qkv, cos, sin, Hq, Hkv, "wmma")
    with pytest.raises(ValueError):
        ops.qkv_attention(qkv, cos, sin, Hq, 3, "ck")


# ---------------------------------------------------------------------------
# (d) the model
# ---------------------------------------------------------------------------
def _model_cfg():
    return LlamaConfig(dim=512, n_layers=2, n_heads=4, n_kv_heads=2,
                       intermediate=1024, vocab_size=512, max_seq_len=256)


def _loss_and_grads(device, dtype, switch, monkeypatch, ckpt=False):
    monkeypatch.setenv("KT_ATTN_PACK", switch)
    torch.manual_seed(7)
    model = Llama(_model_cfg()).to(device=device, dtype=dtype)
    if ckpt:
        model.gradient_checkpointing_enable()
    gen = torch.Generator().manual_seed(8)
    x = torch.randint(0, 512, (2, 256), generator=gen).to(device)
    y = torch.randint(0, 512, (2, 256), generator=gen).to(device)
    loss = model.loss(x, y)
    loss.backward()
    return loss.item(), {n: p.grad for n, p in model.named_parameters()}


def _spy_qkv_attention(monkeypatch):
    """-> list that receives the impl of every ops.qkv_attention call."""
    calls = []
    real = ops.qkv_attention

    def spy(qkv, cos, sin, n_heads, n_kv, impl):
        calls.append(impl)
        return real(qkv, cos, sin, n_heads, n_kv, impl)

    monkeypatch.setattr(ops, "qkv_attention", spy)
    return calls


@pytest.mark.parametrize("impl", ["v3", "ck"])
def test_model_switch_cpu(impl, monkeypatch):
    """A CPU model never passes the kernels' support gates, so they are
    opened here: Attention.forward then calls ops.qkv_attention, which off
    the GPU runs the separate rope nodes around SDPA whatever the switch
    says. Both settings must agree bitwise, and with the model's untouched
    rope + SDPA path up to fp32 rounding (v3 folds scale*log2e into q and
    gives SDPA ln2, SDPA's own path scales the scores).

    Tolerance against the untouched path, per tensor, 1e-3 * max|ref|: an
    fp32 dot product of K <= 1024 terms (the widest layer here) is off by at
    most K * 2^-24 = 6.1e-5 of its magnitude, and about 16 such stages lie
    between the embedding, the loss and the gradient of the first layer;
    16 * 6.1e-5 = 1e-3. A wrong split, scale or rotation is off by the
    magnitude itself."""
    monkeypatch.delenv("KT_ATTN", raising=False)
    calls = _spy_qkv_attention(monkeypatch)
    lr, gr = _loss_and_grads("cpu", torch.float32, "1", monkeypatch)
    assert calls == [], "the untouched CPU model takes rope + SDPA"

    monkeypatch.setattr(ops, "flash_attention_v3_supported",
                        lambda *a, **kw: impl == "v3")
    monkeypatch.setattr(ops, "flash_attention_supported",
                        lambda *a, **kw: True)
    l0, g0 = _loss_and_grads("cpu", torch.float32, "0", monkeypatch)
    assert calls == [impl] * 2, "one qkv_attention call per layer"
    l1, g1 = _loss_and_grads("cpu", torch.float32, "1", monkeypatch)
    assert calls == [impl] * 4

    assert l0 == l1
    assert l1 == pytest.approx(lr, rel=1e-3)
    assert g0.keys() == g1.keys() == gr.keys()
    for n, ref in gr.items():
        assert torch.equal(g0[n], g1[n]), n
        atol = 1e-3 * ref.abs().max().item()
        print(f"{impl} {n}: max diff {(g1[n] - ref).abs().max().item():.3e}"
              f", atol {atol:.3e}")
        torch.testing.assert_close(g1[n], ref, rtol=0, atol=atol, msg=n)


@pytest.mark.gpu
def test_model_switch_gpu(monkeypatch):
    assert _model_cfg().head_dim == 128
    l0, g0 = _loss_and_grads("cuda", BF16, "0", monkeypatch)
    proxy = _CountPackKernel(ops._ext())
    monkeypatch.setattr(ops, "_ext", lambda: proxy)
    l1, g1 = _loss_and_grads("cuda", BF16, "1", monkeypatch)
    assert proxy.calls == 2, "one attn_grad_pack per layer"
    l2, g2 = _loss_and_grads("cuda", BF16, "1", monkeypatch, ckpt=True)
    assert proxy.calls == 4
    assert l0 == l1
    assert l2 == pytest.approx(l0, abs=1e-3)
    for n, ref in g0.items():
        atol = max(2e-2, 6e-3 * ref.float().abs().max().item())
        for tag, got in (("pack", g1[n]), ("pack+ckpt", g2[n])):
            torch.testing.assert_close(got.float(), ref.float(), rtol=2e-2,
                                       atol=atol, msg=f"{n} ({tag})")
