"""kubetorch_amd.ops — MI355X-native fused ops with autograd.

Dispatch policy:
  * GPU tensors run the hand-written gfx950 HIP kernels (_hip_ops.so,
    built in-tree by kubetorch_amd.ops.build). If the extension is missing
    on a GPU box the ops raise — there is no silent eager fallback.
  * CPU tensors run a plain fp32 PyTorch reference of the same op; this is
    the numerics reference the GPU tests compare against, and what CPU-only
    CI exercises.
"""
import importlib.util
import os
import weakref

import torch

_EXT = None
_EXT_ERR = None


def _ext():
    """Load the in-tree HIP extension, raising loudly if unavailable."""
    global _EXT, _EXT_ERR
    if _EXT is not None:
        return _EXT
    if _EXT_ERR is not None:
        raise _EXT_ERR
    so = os.path.join(os.path.dirname(__file__), "_hip_ops.so")
    if not os.path.exists(so):
        _EXT_ERR = RuntimeError(
            f"kubetorch_amd HIP extension not built: {so} missing. "
            "Run `python -m kubetorch_amd.ops.build` (gfx950)."
        )
        raise _EXT_ERR
    spec = importlib.util.spec_from_file_location("kubetorch_amd.ops._hip_ops", so)
    mod = importlib.util.module_from_spec(spec)
    try:
        spec.loader.exec_module(mod)
    except Exception as e:  # pragma: no cover
        _EXT_ERR = RuntimeError(f"failed to load {so}: {e}")
        raise _EXT_ERR
    _EXT = mod
    return _EXT


def hip_available():
    try:
        _ext()
        return True
    except Exception:
        # On a GPU machine a missing extension must FAIL, not silently
        # run the eager fallback at a fraction of the speed (the gfx950
        # .so ships in-tree; its absence means a broken build/snapshot).
        # KT_ALLOW_EAGER_FALLBACK=1 overrides for debugging.
        import torch

        if torch.cuda.is_available() and \
                os.environ.get("KT_ALLOW_EAGER_FALLBACK") != "1":
            raise
        return False


_SPILL = None


def _spill_ext():
    """The native checkpoint spill engine (_hip_spill.so)."""
    global _SPILL
    if _SPILL is not None:
        return _SPILL
    so = os.path.join(os.path.dirname(__file__), "_hip_spill.so")
    if not os.path.exists(so):
        raise RuntimeError(
            f"spill extension not built: {so} missing "
            "(python -m kubetorch_amd.ops.build)")
    spec = importlib.util.spec_from_file_location(
        "kubetorch_amd.ops._hip_spill", so)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    _SPILL = mod
    return _SPILL


# ---------------------------------------------------------------------------
# RMSNorm
# ---------------------------------------------------------------------------
def _rmsnorm_ref_fwd(x, w, eps):
    xf = x.float()
    invrms = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    y = (xf * invrms * w.float()).to(x.dtype)
    return y, invrms.squeeze(-1).reshape(-1)


def _rmsnorm_ref_bwd(dy, ds, s, w, invrms):
    H = s.shape[-1]
    sf = s.float().reshape(-1, H)
    dyf = dy.float().reshape(-1, H)
    wf = w.float()
    ir = invrms.reshape(-1, 1)
    S = (dyf * wf * sf).sum(-1, keepdim=True)
    g = ir * dyf * wf - sf * (ir ** 3) * S / H
    if ds is not None:
        g = g + ds.float().reshape(-1, H)
    dw = (dyf * sf * ir).sum(0).to(w.dtype)
    return g.to(s.dtype).reshape(s.shape), dw


class _RMSNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, eps):
        if x.is_cuda:
            y, invrms = _ext().rmsnorm_fwd(x.contiguous(), None,
                                           w.contiguous(), eps)
        else:
            y, invrms = _rmsnorm_ref_fwd(x, w, eps)
        ctx.save_for_backward(x, w, invrms)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, invrms = ctx.saved_tensors
        if x.is_cuda:
            dx, dw = _ext().rmsnorm_bwd(dy.contiguous(), None, x.contiguous(),
                                        w.contiguous(), invrms)
        else:
            dx, dw = _rmsnorm_ref_bwd(dy, None, x, w, invrms)
        return dx, dw, None


def rmsnorm(x, w, eps=1e-5):
    """y = x * rsqrt(mean(x^2, -1) + eps) * w (bf16 in/out, fp32 accum)."""
    return _RMSNorm.apply(x, w, eps)


class _AddRMSNorm(torch.autograd.Function):
    """Fused pre-norm residual add: (y, s) = (rmsnorm(x + res) * w, x + res).
    Backward folds the residual fan-in add: dx = dres = ds + d(norm)·dy."""

    @staticmethod
    def forward(ctx, x, res, w, eps):
        ctx.set_materialize_grads(False)  # unused s output -> ds is None
        if x.is_cuda:
            y, invrms, s = _ext().rmsnorm_fwd(x.contiguous(), res.contiguous(),
                                              w.contiguous(), eps)
        else:
            s = (x.float() + res.float()).to(x.dtype)
            y, invrms = _rmsnorm_ref_fwd(s, w, eps)
        ctx.save_for_backward(s, w, invrms)
        return y, s

    @staticmethod
    def backward(ctx, dy, ds):
        s, w, invrms = ctx.saved_tensors
        if dy is None:
            dy = torch.zeros_like(s)
        if ds is not None:
            ds = ds.contiguous()
        if s.is_cuda:
            g, dw = _ext().rmsnorm_bwd(dy.contiguous(), ds, s, w.contiguous(),
                                       invrms)
        else:
            g, dw = _rmsnorm_ref_bwd(dy, ds, s, w, invrms)
        return g, g, dw, None


def add_rmsnorm(x, res, w, eps=1e-5):
    """Fused residual add + RMSNorm: returns (normed, x + res)."""
    return _AddRMSNorm.apply(x, res, w, eps)


# ---------------------------------------------------------------------------
# RoPE (Llama rotate-half)
# ---------------------------------------------------------------------------
def precompute_rope(seq_len, head_dim, base=500000.0, device=None):
    """cos/sin tables [S, D/2] fp32 (host-side trig per CDNA guide App. B)."""
    inv_freq = 1.0 / (
        base ** (torch.arange(0, head_dim, 2, dtype=torch.float32, device=device) / head_dim)
    )
    t = torch.arange(seq_len, dtype=torch.float32, device=device)
    freqs = torch.outer(t, inv_freq)  # [S, D/2]
    return freqs.cos().contiguous(), freqs.sin().contiguous()


def _rope_ref(x, cos, sin, sign, oscale=1.0):
    # x: [B, S, Hh, D]
    B, S, Hh, D = x.shape
    xf = x.float()
    x1, x2 = xf[..., : D // 2], xf[..., D // 2 :]
    c = cos[:S].view(1, S, 1, D // 2)
    s = sin[:S].view(1, S, 1, D // 2) * sign
    o1 = (x1 * c - x2 * s) * oscale
    o2 = (x2 * c + x1 * s) * oscale
    return torch.cat([o1, o2], dim=-1).to(x.dtype)


class _Rope(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cos, sin, oscale):
        ctx.S = x.shape[1]
        ctx.oscale = oscale
        ctx.save_for_backward(cos, sin)
        if x.is_cuda:
            B, S, Hh, D = x.shape
            xv = x.reshape(B * S, Hh, D)  # strided views pass through
            return _ext().rope(xv, cos, sin, S, 1.0, oscale).view(x.shape)
        return _rope_ref(x, cos, sin, 1.0, oscale)

    @staticmethod
    def backward(ctx, dy):
        # RoPE is linear: y = oscale * R(x)  =>  dx = oscale * R^T(dy), so
        # the same oscale rides along for free in the backward kernel.
        cos, sin = ctx.saved_tensors
        if dy.is_cuda:
            B, S, Hh, D = dy.shape
            dyv = dy.reshape(B * S, Hh, D)
            dx = _ext().rope(dyv, cos, sin, S, -1.0, ctx.oscale).view(dy.shape)
        else:
            dx = _rope_ref(dy, cos, sin, -1.0, ctx.oscale)
        return dx, None, None, None


def rope(x, cos, sin, oscale=1.0):
    """Apply rotate-half RoPE to x: [B, S, Hh, D] using [S, D/2] tables.

    oscale multiplies the output in fp32 before the bf16 round (free in the
    memory-bound kernel). Used to fold the attention softmax scale * log2e
    into Q for the v3 FMHA path (flash_attention impl="v3")."""
    return _Rope.apply(x, cos, sin, oscale)


# ---------------------------------------------------------------------------
# SwiGLU
# ---------------------------------------------------------------------------
def _swiglu_ref_fwd(gu):
    I = gu.shape[-1] // 2
    g, u = gu[..., :I].float(), gu[..., I:].float()
    return (torch.nn.functional.silu(g) * u).to(gu.dtype)


class _SwiGLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gu):
        ctx.save_for_backward(gu)
        if gu.is_cuda:
            return _ext().swiglu_fwd(gu.contiguous())
        return _swiglu_ref_fwd(gu)

    @staticmethod
    def backward(ctx, dout):
        (gu,) = ctx.saved_tensors
        if gu.is_cuda:
            return _ext().swiglu_bwd(dout.contiguous(), gu.contiguous())
        I = gu.shape[-1] // 2
        g, u = gu[..., :I].float(), gu[..., I:].float()
        do = dout.float()
        sig = torch.sigmoid(g)
        dg = do * u * sig * (1 + g * (1 - sig))
        du = do * g * sig
        return torch.cat([dg, du], dim=-1).to(gu.dtype)


def swiglu(gate_up):
    """out = silu(gate) * up with gate_up = [..., 2I] packed from one GEMM."""
    return _SwiGLU.apply(gate_up)


# ---------------------------------------------------------------------------
# Fused cross entropy (destroys logits: overwritten with the gradient)
# ---------------------------------------------------------------------------
class _FusedCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets, ignore_index):
        V = logits.shape[-1]
        flat = logits.reshape(-1, V)
        t = targets.reshape(-1)
        n_valid = (t != ignore_index).sum().clamp(min=1)
        if logits.is_cuda:
            loss = _ext().cross_entropy_fwd_(flat, t.contiguous(), 1.0, ignore_index)
            dlogits = flat  # overwritten in place by the kernel
        else:
            lf = flat.float()
            logp = torch.log_softmax(lf, dim=-1)
            loss = torch.nn.functional.nll_loss(
                logp, t, reduction="none", ignore_index=ignore_index
            )
            dlogits = torch.softmax(lf, dim=-1)
            valid = (t != ignore_index).unsqueeze(-1)
            dlogits.scatter_add_(
                1, t.clamp(min=0).unsqueeze(1), -torch.ones_like(t, dtype=torch.float32).unsqueeze(1)
            )
            dlogits = torch.where(valid, dlogits, torch.zeros_like(dlogits)).to(logits.dtype)
        ctx.save_for_backward(dlogits, n_valid)
        ctx.shape = logits.shape
        return loss.sum() / n_valid.to(loss.dtype)

    @staticmethod
    def backward(ctx, gout):
        dlogits, n_valid = ctx.saved_tensors
        scale = (gout / n_valid).to(torch.float32)
        if dlogits.is_cuda:
            # a bf16 tensor times a 0-dim GPU tensor would round the factor
            # itself to bf16; the kernel multiplies in fp32 and rounds once
            g = _ext().scale_bf16(dlogits, scale.reshape(1))
        else:
            g = (dlogits * scale).to(dlogits.dtype)
        return g.reshape(ctx.shape), None, None


def fused_cross_entropy(logits, targets, ignore_index=-100):
    """Mean CE over valid tokens. WARNING: logits buffer is overwritten with
    the (unscaled) gradient on GPU — do not reuse logits after this call."""
    return _FusedCE.apply(logits, targets, ignore_index)


# ---------------------------------------------------------------------------
# Flash attention: custom gfx950 forward + torch (AITER asm) backward
# ---------------------------------------------------------------------------
_LN2 = 0.6931471805599453
LOG2E = 1.4426950408889634


def _attention_forward(q, k, v, scale, impl):
    """-> (q, k, v as saved for backward, o, lse, effective scale)."""
    if impl == "v3":
        # AITER-schedule CK v3 kernel (fastest fwd, profiles/). Contract:
        # q arrives PRE-SCALED by scale*log2e (folded into the RoPE
        # kernel's oscale), so softmax(scale*q0@kT) == softmax(ln2*q@kT)
        # and the effective scale for fwd LSE and backward is ln2.
        o, lse = _ext().attn_fwd_v3(q, k, v, scale, prescaled=True)
        scale = _LN2
    elif impl == "ck":
        # CK path is stride-aware: permuted [B,S,H,D] views go in as-is
        o, lse = _ext().attn_fwd_ck_tr(q, k, v, scale)
    else:
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        o, lse = _ext().attn_fwd(q, k, v, scale)
    return q, k, v, o, lse, scale


def _attention_backward_expanded(grad_out, q, k, v, o, lse, scale):
    """Dense backward -> (dq, dk_e, dv_e), all [B, Hq, S, D]: dk_e and dv_e
    are per query head (expanded head h belongs to kv head h // g) and still
    have to be summed over each group."""
    B, Hq, S, D = q.shape
    g = Hq // k.shape[1]
    if os.environ.get("KT_ATTN_BWD") == "ck" and S % 128 == 0:
        # Opt-in: CK-tile GQA-native bwd (no KV expansion; dk/dv come
        # back Hq-expanded and are group-summed). Numerically validated
        # on gfx950 (tests/test_ops.py::test_attn_bwd_ck_gqa_native);
        # measured 4.42 ms vs 2.99 ms for the aten/AITER-asm path at the
        # Llama-3-8B shape (B4 H32/8 S4096), so aten stays the default
        # hot path — see profiles/ROUND2.md lever #1.
        return tuple(_ext().attn_bwd_ck(
            grad_out.contiguous(), q.contiguous(), k.contiguous(),
            v.contiguous(), o.contiguous(), lse.contiguous(), scale))
    if g > 1:  # expand KV for the dense backward, then reduce over groups
        k_exp = k.repeat_interleave(g, dim=1)
        v_exp = v.repeat_interleave(g, dim=1)
    else:
        k_exp, v_exp = k, v
    seed = torch.zeros((), dtype=torch.long, device=q.device)
    offset = torch.zeros((), dtype=torch.long, device=q.device)
    dq, dk_e, dv_e, _ = \
        torch.ops.aten._scaled_dot_product_efficient_attention_backward(
            grad_out, q, k_exp, v_exp, None, o, lse, seed, offset,
            0.0, [True, True, True, False], True, scale=scale,
        )
    return dq, dk_e, dv_e


class _FlashAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, scale, impl):
        q, k, v, o, lse, scale = _attention_forward(q, k, v, scale, impl)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.scale = scale
        return o

    @staticmethod
    def backward(ctx, grad_out):
        q, k, v, o, lse = ctx.saved_tensors
        B, Hq, S, D = q.shape
        Hkv = k.shape[1]
        g = Hq // Hkv
        dq, dk, dv = _attention_backward_expanded(
            grad_out.contiguous(), q, k, v, o, lse, ctx.scale)
        if g > 1:
            dk = dk.view(B, Hkv, g, S, D).sum(2)
            dv = dv.view(B, Hkv, g, S, D).sum(2)
        return dq, dk, dv, None, None


def flash_attention(q, k, v, scale=None, impl="ck"):
    """Causal GQA attention fwd, bf16, D=128, layout [B, H, S, D], paired
    with torch's AITER asm backward. impl="ck" (default) runs the CK-tile
    FMHA tr-load instantiation (1.8x AOTriton on the Llama shape —
    profiles/); impl="v3" runs the AITER-schedule v3 kernel (2.0x) and
    REQUIRES q pre-scaled by scale*log2e (fold it into ops.rope's oscale);
    impl="wmma" runs the in-tree rocWMMA kernel (ops/hip/attention.hip,
    requires S % 128 == 0)."""
    if impl not in ("ck", "v3", "wmma"):
        raise ValueError(f'impl must be "ck", "v3" or "wmma", got {impl!r}')
    if scale is None:
        scale = q.shape[-1] ** -0.5
    return _FlashAttention.apply(q, k, v, scale, impl)


def flash_attention_supported(q, k, v, is_causal):
    return (is_causal and q.is_cuda and q.dtype == torch.bfloat16
            and q.shape[-1] == 128 and q.shape[2] % 128 == 0
            and q.shape[2] >= 256 and hip_available())


def flash_attention_v3_supported(S, head_dim, device, dtype):
    """Shape gate for the v3 (prescaled-Q) path, checkable BEFORE RoPE so
    the softmax scale can be folded into the RoPE output."""
    return (head_dim == 128 and S % 256 == 0 and S >= 256
            and device.type == "cuda" and dtype == torch.bfloat16
            and hip_available())


# ---------------------------------------------------------------------------
# Attention block as one autograd node: qkv split + RoPE + flash attention
# forward; dense backward + one kernel for GQA sum, RoPE^T and qkv packing
# ---------------------------------------------------------------------------
def attn_pack_enabled():
    """KT_ATTN_PACK=0 restores the separate rope / attention / sum / cat
    autograd nodes, so one tree can run an A/B."""
    return os.environ.get("KT_ATTN_PACK", "1") != "0"


def _rope_bwd(dy, cos, sin, oscale):
    # dy: [B, S, Hh, D], any layout (the GPU reshape copies if it must)
    if dy.is_cuda:
        B, S, Hh, D = dy.shape
        return _ext().rope(dy.reshape(B * S, Hh, D), cos, sin, S, -1.0,
                           oscale).view(dy.shape)
    return _rope_ref(dy, cos, sin, -1.0, oscale)


def _attn_grad_pack_ref(dq, dk_e, dv_e, cos, sin, n_kv, q_oscale):
    """The composition attn_grad_pack replaces: bf16 group sums, the rope
    backward on dq and dk, and the cat into qkv column order. It rounds the
    k part twice (after the sum and after the rotation)."""
    B, Hq, S, D = dq.shape
    g = Hq // n_kv
    if g > 1:
        dk = dk_e.reshape(B, n_kv, g, S, D).sum(2)
        dv = dv_e.reshape(B, n_kv, g, S, D).sum(2)
    else:
        dk, dv = dk_e, dv_e
    dq = _rope_bwd(dq.transpose(1, 2), cos, sin, q_oscale)
    dk = _rope_bwd(dk.transpose(1, 2), cos, sin, 1.0)
    return torch.cat([dq.reshape(B, S, Hq * D), dk.reshape(B, S, n_kv * D),
                      dv.transpose(1, 2).reshape(B, S, n_kv * D)], dim=-1)


def _attn_grad_pack_kernel_ok(dq, dk_e, dv_e, cos, sin):
    """The binding's layout checks (it raises where this returns False)."""
    for t in (dq, dk_e, dv_e):
        if not (t.is_cuda and t.dtype == torch.bfloat16
                and t.device == dq.device and t.stride(3) == 1
                and t.data_ptr() % 16 == 0):
            return False
        if any(t.shape[d] != 1 and (t.stride(d) < 0 or t.stride(d) % 8)
               for d in range(3)):
            return False
    for t in (cos, sin):
        if not (t.is_cuda and t.device == dq.device
                and t.dtype == torch.float32 and t.is_contiguous()
                and t.data_ptr() % 16 == 0):
            return False
    return dq.shape[3] % 8 == 0


def attn_grad_pack(dq, dk_e, dv_e, cos, sin, n_kv, q_oscale=1.0):
    """dqkv [B, S, (Hq + 2*n_kv)*D] from the dense attention backward's
    (dq, dk_e, dv_e), each bf16 [B, Hq, S, D] with dk_e/dv_e per query head:

        q part = q_oscale * R^T(dq)
        k part = R^T(sum_j dk_e[kv*g + j])      g = Hq // n_kv
        v part = sum_j dv_e[kv*g + j]

    R^T is the rope backward at position s with the fp32 [>=S, D/2] cos/sin
    tables. On the GPU one kernel does it in fp32 with a single bf16 round
    per element; [B,H,S,D] buffers and transposed [B,S,H,D] buffers both go
    in without a copy. On CPU, and for layouts the kernel does not take, the
    separate sum / rope / cat composition runs instead."""
    if dq.dim() != 4 or dk_e.shape != dq.shape or dv_e.shape != dq.shape:
        raise ValueError("dq, dk_e and dv_e must be equal-shaped "
                         "[B, Hq, S, D]")
    B, Hq, S, D = dq.shape
    if n_kv < 1 or Hq % n_kv:
        raise ValueError(f"Hq={Hq} is not a multiple of n_kv={n_kv}")
    if D % 2 or cos.dim() != 2 or cos.shape != sin.shape \
            or cos.shape[0] < S or cos.shape[1] != D // 2:
        raise ValueError("cos/sin must be [>=S, D/2] tables")
    if _attn_grad_pack_kernel_ok(dq, dk_e, dv_e, cos, sin):
        return _ext().attn_grad_pack(dq, dk_e, dv_e, cos, sin, n_kv,
                                     q_oscale)
    return _attn_grad_pack_ref(dq, dk_e, dv_e, cos[:S], sin[:S], n_kv,
                               q_oscale)


def _qkv_split_rope(qkv, cos, sin, n_heads, n_kv, impl):
    """-> rotated q [B,Hq,S,D], rotated k and raw v [B,Hkv,S,D] as views of
    [B,S,H,D] buffers, and the scale folded into q (v3: scale*log2e)."""
    B, S, W = qkv.shape
    hd = W // (n_heads + 2 * n_kv)
    q, k, v = qkv.split([n_heads * hd, n_kv * hd, n_kv * hd], dim=-1)
    q_oscale = (hd ** -0.5) * LOG2E if impl == "v3" else 1.0
    q = rope(q.view(B, S, n_heads, hd), cos, sin, oscale=q_oscale)
    k = rope(k.view(B, S, n_kv, hd), cos, sin)
    v = v.view(B, S, n_kv, hd)
    q, k, v = (t.transpose(1, 2) for t in (q, k, v))
    return q, k, v, q_oscale


class _QKVAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, cos, sin, n_heads, n_kv, impl):
        B, S, _ = qkv.shape
        q, k, v, q_oscale = _qkv_split_rope(qkv, cos, sin, n_heads, n_kv,
                                            impl)
        q, k, v, o, lse, scale = _attention_forward(
            q, k, v, q.shape[-1] ** -0.5, impl)
        ctx.save_for_backward(q, k, v, o, lse, cos, sin)
        ctx.scale, ctx.q_oscale, ctx.n_kv = scale, q_oscale, n_kv
        return o.transpose(1, 2).reshape(B, S, -1)

    @staticmethod
    def backward(ctx, grad_out):
        q, k, v, o, lse, cos, sin = ctx.saved_tensors
        B, Hq, S, D = q.shape
        # the [B,H,S,D] view of the [B,S,H*D] gradient goes in strided, the
        # way o does: the dense backward wants it token-major anyway
        grad_out = grad_out.reshape(B, S, Hq, D).transpose(1, 2)
        dq, dk_e, dv_e = _attention_backward_expanded(
            grad_out, q, k, v, o, lse, ctx.scale)
        dqkv = attn_grad_pack(dq, dk_e, dv_e, cos, sin, ctx.n_kv,
                              ctx.q_oscale)
        return dqkv, None, None, None, None, None


def qkv_attention(qkv, cos, sin, n_heads, n_kv, impl="ck"):
    """Causal GQA attention block between the wqkv and wo GEMMs: qkv
    [B, S, (n_heads + 2*n_kv)*D] (the wqkv output) -> o [B, S, n_heads*D].
    Splits qkv, rotates q and k (impl="v3" folds scale*log2e into q) and runs
    flash_attention's forward kernel; impl is "v3" or "ck".

    As one autograd node its backward is the dense attention backward
    followed by attn_grad_pack, which returns dqkv directly. KT_ATTN_PACK=0
    runs the separate rope / flash_attention nodes instead; on CPU those
    run with SDPA in place of the forward kernel."""
    if impl not in ("v3", "ck"):
        raise ValueError('impl must be "v3" or "ck"')
    if qkv.dim() != 3 or qkv.shape[-1] % (n_heads + 2 * n_kv) \
            or n_heads % n_kv:
        raise ValueError("qkv must be [B, S, (n_heads + 2*n_kv)*D] with "
                         "n_heads a multiple of n_kv")
    if qkv.is_cuda and attn_pack_enabled():
        return _QKVAttention.apply(qkv, cos, sin, n_heads, n_kv, impl)
    B, S, _ = qkv.shape
    q, k, v, _ = _qkv_split_rope(qkv, cos, sin, n_heads, n_kv, impl)
    if qkv.is_cuda:
        o = flash_attention(q, k, v, impl=impl)
    else:
        g = n_heads // n_kv
        o = torch.nn.functional.scaled_dot_product_attention(
            q, k.repeat_interleave(g, 1), v.repeat_interleave(g, 1),
            is_causal=True,
            scale=_LN2 if impl == "v3" else q.shape[-1] ** -0.5)
    return o.transpose(1, 2).reshape(B, S, -1)


# ---------------------------------------------------------------------------
# Paged KV cache (serving decode): page write + single-token attention.
# Inference-only, no autograd. Pools are [num_pages, n_kv, page_size, hd].
# ---------------------------------------------------------------------------
PAGED_PAGE_SIZES = (16, 32, 64)
PAGED_HEAD_DIMS = (64, 128)
PAGED_GROUPS = (1, 2, 4, 8)


def _no_grad_inputs(name, *tensors):
    if any(t.requires_grad for t in tensors):
        raise RuntimeError(f"{name} is inference-only: an input requires grad")


def _check_pools(k_pages, v_pages):
    if k_pages.dim() != 4 or v_pages.shape != k_pages.shape:
        raise ValueError("k_pages/v_pages must be equal-shaped "
                         "[num_pages, n_kv, page_size, hd]")
    if not (k_pages.is_contiguous() and v_pages.is_contiguous()):
        raise ValueError("k_pages/v_pages must be contiguous")
    if k_pages.shape[2] not in PAGED_PAGE_SIZES:
        raise ValueError(f"page_size must be one of {PAGED_PAGE_SIZES}")
    if k_pages.shape[3] not in PAGED_HEAD_DIMS:
        raise ValueError(f"head_dim must be one of {PAGED_HEAD_DIMS}")


# fp8 pools: the same layout with torch.float8_e4m3fn (OCP e4m3) elements
# and static fp32 scales per kv head, k_scale / v_scale [n_kv] on the pools'
# device (None = 1.0). A stored byte encodes x / scale, the value read back
# is float(byte) * scale. The kernels read the scales from device memory:
# no host sync, capturable.
PAGED_FP8 = torch.float8_e4m3fn
PAGED_FP8_MAX = 448.0
_FLOAT8_DTYPES = tuple(getattr(torch, n) for n in (
    "float8_e4m3fn", "float8_e5m2", "float8_e4m3fnuz", "float8_e5m2fnuz")
    if hasattr(torch, n))


def _fp8_pools(k_pages, v_pages, k_scale, v_scale):
    """True for a pair of e4m3 pools (the fp8 path), False for unquantised
    pools (the code as it was). One fp8 pool next to another dtype, an
    e5m2 or fnuz pool, and scales without fp8 pools raise."""
    kd, vd = k_pages.dtype, v_pages.dtype
    if kd == PAGED_FP8 and vd == PAGED_FP8:
        return True
    if kd in _FLOAT8_DTYPES or vd in _FLOAT8_DTYPES:
        raise ValueError("8-bit pools must both be torch.float8_e4m3fn, got "
                         f"{kd} and {vd}")
    if k_scale is not None or v_scale is not None:
        raise ValueError("k_scale/v_scale are for float8_e4m3fn pools only")
    return False


def _fp8_scales(k_pages, k_scale, v_scale):
    """The two [n_kv] fp32 scale tensors of an fp8 pool pair, None replaced
    by ones. Shape, dtype and device are checked everywhere; the values
    (positive, finite) only on the CPU, where looking is no device sync."""
    n_kv = k_pages.shape[1] if k_pages.dim() == 4 else -1
    out = []
    for name, s in (("k_scale", k_scale), ("v_scale", v_scale)):
        if s is None:
            s = torch.ones(max(n_kv, 0), dtype=torch.float32,
                           device=k_pages.device)
        if not torch.is_tensor(s) or s.dtype != torch.float32 \
                or tuple(s.shape) != (n_kv,) or s.device != k_pages.device:
            raise ValueError(f"{name} must be [n_kv] fp32 on the pools' "
                             "device")
        if not s.is_cuda and not bool(((s > 0) & s.isfinite()).all()):
            raise ValueError(f"{name} must be positive and finite")
        out.append(s.contiguous())
    return out


_INV_SCALES = {}   # id(scale) -> (weakref, version, 1/scale)


def _inv_scale(s):
    """s.reciprocal(), kept per scale tensor while it lives and is not
    written in place: the serving engine passes the same static scales in
    every step of every layer, and two more launches per paged_kv_write
    cost a decode step more than the fp8 read saves it."""
    key = id(s)
    hit = _INV_SCALES.get(key)
    if hit is not None and hit[0]() is s and hit[1] == s._version:
        return hit[2]
    inv = s.reciprocal()
    if s.is_cuda and torch.cuda.is_current_stream_capturing():
        return inv  # lives in the graph's memory pool: not kept
    _INV_SCALES[key] = (weakref.ref(s, lambda _: _INV_SCALES.pop(key, None)),
                        s._version, inv)
    return inv


def _fp8_quantize_ref(x, inv_scale):
    """[T, n_kv, hd] -> e4m3: one fp32 multiply by the head's 1/scale, clamp
    to the finite range, round to nearest even. NaN stays NaN, +-inf
    saturate. The kernel's bytes equal this."""
    y = x.float() * inv_scale.view(1, -1, 1)
    return y.clamp(-PAGED_FP8_MAX, PAGED_FP8_MAX).to(PAGED_FP8)


def paged_kv_write(k_new, v_new, k_pages, v_pages, slot_mapping,
                   k_scale=None, v_scale=None):
    """Scatter k_new/v_new [T, n_kv, hd] into the page pools in place.

    slot_mapping [T] int32 holds each token's flat physical index
    page*page_size + offset; a negative entry writes nothing. The result is
    bitwise what a torch indexed copy gives. Into float8_e4m3fn pools the
    rows are quantised with k_scale/v_scale ([n_kv] fp32, None = 1.0):
    bitwise _fp8_quantize_ref."""
    _no_grad_inputs("paged_kv_write", k_new, v_new, k_pages, v_pages)
    fp8 = _fp8_pools(k_pages, v_pages, k_scale, v_scale)
    k_inv = v_inv = None
    if fp8:
        k_inv, v_inv = (_inv_scale(s) for s in
                        _fp8_scales(k_pages, k_scale, v_scale))
    if k_pages.is_cuda:
        _ext().paged_kv_write(k_new, v_new, k_pages, v_pages, slot_mapping,
                              k_inv, v_inv)
        return
    _check_pools(k_pages, v_pages)
    P, Hkv, ps, hd = k_pages.shape
    if (k_new.shape != v_new.shape or k_new.dim() != 3
            or tuple(k_new.shape[1:]) != (Hkv, hd)):
        raise ValueError("k_new/v_new must be [T, n_kv, hd] matching the pool")
    if slot_mapping.dtype != torch.int32 or \
            tuple(slot_mapping.shape) != (k_new.shape[0],):
        raise ValueError("slot_mapping must be [T] int32")
    slots = slot_mapping.long()
    keep = (slots >= 0) & (slots < P * ps)
    page, off = slots[keep] // ps, slots[keep] % ps
    if fp8:
        if k_new.dtype not in (torch.bfloat16, torch.float32) \
                or v_new.dtype != k_new.dtype:
            raise ValueError("k_new/v_new must be bf16 (fp32 on the CPU "
                             "reference path)")
        k_pages[page, :, off] = _fp8_quantize_ref(k_new[keep], k_inv)
        v_pages[page, :, off] = _fp8_quantize_ref(v_new[keep], v_inv)
        return
    k_pages[page, :, off] = k_new[keep].to(k_pages.dtype)
    v_pages[page, :, off] = v_new[keep].to(v_pages.dtype)


# Workgroup target of the split heuristic: two workgroups for each of the
# MI355X's 256 CUs. A workgroup's loop loads a chunk, then computes on it,
# so a second resident workgroup is what keeps loads in flight meanwhile.
# Measured at the 8B shape (Hq 32, Hkv 8, hd 128, page 16; kernel + merge,
# profiles/paged_decode.json "split_sweep"): batch 8 x 4,160 tokens is
# fastest at 8-12 splits (512-768 workgroups, 39-40 us against 48 us at 4
# and 47 us at 16), batch 32 x 2,048 at 2-8 splits (65-67 us against 83 us
# at 1), batch 1 x 8,192 still gains up to 32 splits.
# _PAGED_MIN_TOKENS_PER_SPLIT keeps a split at four 64-token chunks of the
# kernel's main loop (16 pages of 16): in the same sweep 260 tokens per
# split (16 splits of 4,160) is already slower than 347, and at 200 tokens
# a second split does not pay at batch 32.
_PAGED_TARGET_WORKGROUPS = 512
_PAGED_MIN_TOKENS_PER_SPLIT = 256
_PAGED_MAX_SPLITS = 32


def paged_num_splits(batch, n_kv, max_tokens):
    """Split-KV factor for paged_attention_decode(num_splits=0): enough
    workgroups to cover the CUs at small batch*n_kv, capped so one split
    keeps a few pages of the longest possible sequence."""
    want = -(-_PAGED_TARGET_WORKGROUPS // max(1, batch * n_kv))
    cap = max(1, max_tokens // _PAGED_MIN_TOKENS_PER_SPLIT)
    return max(1, min(want, cap, _PAGED_MAX_SPLITS))


def _dequant(rows, kv_scale):
    """Gathered pool rows [n, Hkv, hd] -> fp32 [Hkv, n, hd]; fp8 rows are
    multiplied by their kv head's scale (kv_scale [Hkv], None otherwise)."""
    x = rows.float().transpose(0, 1)
    return x if kv_scale is None else x * kv_scale.view(-1, 1, 1)


def _paged_attention_ref(q, k_pages, v_pages, block_table, seq_lens, scale,
                         k_scale=None, v_scale=None):
    """fp32 reference: per sequence, gather the valid tokens through the
    block table and run softmax(q k^T scale) v. Pages that are not
    referenced and positions >= seq_len are never indexed."""
    B, Hq, hd = q.shape
    P, Hkv, ps, _ = k_pages.shape
    g = Hq // Hkv
    max_tokens = block_table.shape[1] * ps
    out = torch.zeros(B, Hq, hd, dtype=torch.float32, device=q.device)
    lens = seq_lens.tolist()
    table = block_table.tolist()
    for b in range(B):
        n = max(0, min(int(lens[b]), max_tokens))
        toks = [(table[b][t // ps], t % ps) for t in range(n)]
        toks = [(p, o) for p, o in toks if 0 <= p < P]
        if not toks:
            continue
        page = torch.tensor([p for p, _ in toks], device=q.device)
        off = torch.tensor([o for _, o in toks], device=q.device)
        k = _dequant(k_pages[page, :, off], k_scale)        # [Hkv, n, hd]
        v = _dequant(v_pages[page, :, off], v_scale)
        qb = q[b].float().view(Hkv, g, hd)
        p = torch.softmax(torch.matmul(qb, k.transpose(1, 2)) * scale, dim=-1)
        out[b] = torch.matmul(p, v).view(Hq, hd)
    return out.to(q.dtype)


def paged_attention_decode(q, k_pages, v_pages, block_table, seq_lens,
                           scale=None, num_splits=0, k_scale=None,
                           v_scale=None):
    """Single-token GQA attention over a block-table paged KV cache.

    q [B, Hq, hd]; block_table [B, max_blocks] int32 (-1 = unused);
    seq_lens [B] int32 = valid tokens per row including the one just
    written; a row with seq_lens 0 gives zeros. Reads are proportional to
    each row's own length. num_splits=0 picks a split-KV factor from the
    table's capacity (paged_num_splits); any fixed value gives the same
    result up to fp32 merge rounding. The pools share q's dtype, or are
    both float8_e4m3fn with k_scale/v_scale [n_kv] fp32 (None = 1.0)."""
    _no_grad_inputs("paged_attention_decode", q, k_pages, v_pages)
    fp8 = _fp8_pools(k_pages, v_pages, k_scale, v_scale)
    if fp8:
        k_scale, v_scale = _fp8_scales(k_pages, k_scale, v_scale)
    if scale is None:
        scale = q.shape[-1] ** -0.5
    if num_splits == 0 and k_pages.dim() == 4 and block_table.dim() == 2 \
            and q.dim() == 3:
        num_splits = paged_num_splits(
            q.shape[0], k_pages.shape[1],
            block_table.shape[1] * k_pages.shape[2])
    if q.is_cuda:
        return _ext().paged_attention_decode(q, k_pages, v_pages, block_table,
                                             seq_lens, float(scale),
                                             int(num_splits), k_scale,
                                             v_scale)
    _check_pools(k_pages, v_pages)
    if q.dim() != 3 or q.shape[2] != k_pages.shape[3]:
        raise ValueError("q must be [B, Hq, hd] with the pool's head_dim")
    Hq, Hkv = q.shape[1], k_pages.shape[1]
    if Hq % Hkv or Hq // Hkv not in PAGED_GROUPS:
        raise ValueError(f"group Hq/Hkv must be one of {PAGED_GROUPS}")
    if fp8:
        if q.dtype not in (torch.bfloat16, torch.float32):
            raise ValueError("q must be bf16 (fp32 on the CPU reference path)")
    elif q.dtype != k_pages.dtype or q.dtype != v_pages.dtype:
        raise ValueError("q and the pools must share a dtype")
    if block_table.dtype != torch.int32 or seq_lens.dtype != torch.int32 \
            or block_table.dim() != 2 or block_table.shape[0] != q.shape[0] \
            or tuple(seq_lens.shape) != (q.shape[0],):
        raise ValueError("block_table [B, max_blocks] and seq_lens [B] "
                         "must be int32")
    if num_splits < 1:
        raise ValueError("num_splits must be >= 0")
    return _paged_attention_ref(q, k_pages, v_pages, block_table, seq_lens,
                                float(scale), k_scale, v_scale)


def _paged_prefill_ref(q, k_pages, v_pages, block_table, cu_q_lens, seq_lens,
                       scale, k_scale=None, v_scale=None):
    """fp32 reference of paged_attention_prefill: per row, gather the keys
    the row's query tokens may attend through the block table and run an
    offset-causal softmax. Keys behind table entries outside [0, P) are
    masked, never indexed; a row with more query tokens than seq_lens[b],
    tokens at a position >= max_blocks*page_size and tokens at an index
    outside [0, T) stay zero."""
    T, Hq, hd = q.shape
    P, Hkv, ps, _ = k_pages.shape
    g = Hq // Hkv
    cap = block_table.shape[1] * ps
    out = torch.zeros(T, Hq, hd, dtype=torch.float32, device=q.device)
    cu = cu_q_lens.tolist()
    lens = seq_lens.tolist()
    table = block_table.tolist()
    for b in range(len(lens)):
        qlen = cu[b + 1] - cu[b]
        ctx = lens[b] - qlen
        if ctx < 0:
            continue
        # (query token, position) pairs that are computed at all
        toks = [(cu[b] + i, ctx + i) for i in range(max(0, qlen))
                if ctx + i < cap and 0 <= cu[b] + i < T]
        if not toks:
            continue
        n = max(pos for _, pos in toks) + 1
        pages = [table[b][t // ps] for t in range(n)]
        ok = torch.tensor([0 <= p < P for p in pages], device=q.device)
        page = torch.tensor([p if 0 <= p < P else 0 for p in pages],
                            device=q.device)
        off = torch.arange(n, device=q.device) % ps
        k = _dequant(k_pages[page, :, off], k_scale)        # [Hkv, n, hd]
        v = _dequant(v_pages[page, :, off], v_scale)
        k = torch.where(ok.view(1, n, 1), k, torch.zeros_like(k))
        v = torch.where(ok.view(1, n, 1), v, torch.zeros_like(v))
        ti = torch.tensor([t for t, _ in toks], device=q.device)
        pos = torch.tensor([p for _, p in toks], device=q.device)
        qb = q[ti].float().view(len(toks), Hkv, g, hd).permute(1, 0, 2, 3)
        s = torch.matmul(qb.reshape(Hkv, -1, hd), k.transpose(1, 2)) * scale
        s = s.view(Hkv, len(toks), g, n)
        see = ok.view(1, n) & (torch.arange(n, device=q.device).view(1, n)
                               <= pos.view(-1, 1))          # [toks, n]
        s = s.masked_fill(~see.view(1, len(toks), 1, n), float("-inf"))
        p = torch.softmax(s, dim=-1)
        # a token none of whose keys is readable: zeros, not NaN
        p = torch.where(see.any(1).view(1, -1, 1, 1), p, torch.zeros_like(p))
        o = torch.matmul(p.view(Hkv, -1, n), v).view(Hkv, len(toks), g, hd)
        out[ti] = o.permute(1, 0, 2, 3).reshape(len(toks), Hq, hd)
    return out.to(q.dtype)


def paged_attention_prefill(q, k_pages, v_pages, block_table, cu_q_lens,
                            seq_lens, max_q_len, scale=None, k_scale=None,
                            v_scale=None):
    """Causal GQA attention of a packed, variable-length batch of query
    tokens over a block-table paged KV cache.

    q [T, Hq, hd] packed rows (may be a strided view of the qkv GEMM
    output); block_table [B, max_blocks] int32; cu_q_lens [B+1] int32
    cumulative query counts, row b owns tokens cu[b] .. cu[b+1]-1; seq_lens
    [B] int32 = the row's valid tokens including this call's query tokens,
    whose K/V are already in the pages; max_q_len: host int >= every row's
    query count. Token i of row b sits at position seq_lens[b] - qlen_b + i
    and attends keys [0, position]. Returns [T, Hq, hd]; a row with
    qlen_b > seq_lens[b], tokens at a position >= max_blocks*page_size and
    tokens of no row are zero. The pools share q's dtype, or are both
    float8_e4m3fn with k_scale/v_scale [n_kv] fp32 (None = 1.0)."""
    _no_grad_inputs("paged_attention_prefill", q, k_pages, v_pages)
    fp8 = _fp8_pools(k_pages, v_pages, k_scale, v_scale)
    if fp8:
        k_scale, v_scale = _fp8_scales(k_pages, k_scale, v_scale)
    if scale is None:
        scale = q.shape[-1] ** -0.5
    if q.is_cuda:
        return _ext().paged_attention_prefill(q, k_pages, v_pages,
                                              block_table, cu_q_lens,
                                              seq_lens, int(max_q_len),
                                              float(scale), k_scale, v_scale)
    _check_pools(k_pages, v_pages)
    if q.dim() != 3 or q.shape[2] != k_pages.shape[3]:
        raise ValueError("q must be [T, Hq, hd] with the pool's head_dim")
    Hq, Hkv = q.shape[1], k_pages.shape[1]
    if Hq % Hkv or Hq // Hkv not in PAGED_GROUPS:
        raise ValueError(f"group Hq/Hkv must be one of {PAGED_GROUPS}")
    if q.dtype != torch.bfloat16 and q.dtype != torch.float32:
        raise ValueError("q must be bf16 (fp32 on the CPU reference path)")
    if not fp8 and (q.dtype != k_pages.dtype or q.dtype != v_pages.dtype):
        raise ValueError("q and the pools must share a dtype")
    if block_table.dtype != torch.int32 or block_table.dim() != 2:
        raise ValueError("block_table must be [B, max_blocks] int32")
    B = block_table.shape[0]
    if cu_q_lens.dtype != torch.int32 or tuple(cu_q_lens.shape) != (B + 1,):
        raise ValueError("cu_q_lens must be [B+1] int32")
    if seq_lens.dtype != torch.int32 or tuple(seq_lens.shape) != (B,):
        raise ValueError("seq_lens must be [B] int32")
    if max_q_len < 0:
        raise ValueError("max_q_len must be >= 0")
    if not 0 < scale < float("inf"):
        raise ValueError("scale must be positive and finite")
    return _paged_prefill_ref(q, k_pages, v_pages, block_table, cu_q_lens,
                              seq_lens, float(scale), k_scale, v_scale)


# ---------------------------------------------------------------------------
# Batched token sampling (serving decode): temperature, top-k, top-p and a
# seeded draw per row. Inference-only, no autograd, no host sync.
# ---------------------------------------------------------------------------
SAMPLER_MAX_VOCAB = 262144
_M32 = 0xFFFFFFFF


def _mulhilo32(m, c):
    """(high, low) 32-bit words of m * c for a constant m < 2^32 and an
    int64 tensor c of values < 2^32, without leaving int64: c goes in as
    two 16-bit halves."""
    a = m * (c >> 16)          # < 2^48
    b = m * (c & 0xFFFF)       # < 2^48
    t = ((a & 0xFFFF) << 16) + b
    return (a >> 16) + (t >> 32), t & _M32


def philox4x32_10(counter, key):
    """Philox4x32-10 on int64 tensors of 32-bit words: counter [..., 4],
    key [..., 2] -> [..., 4]. Matches the Random123 known answers."""
    c0, c1, c2, c3 = (counter[..., i] for i in range(4))
    k0, k1 = key[..., 0], key[..., 1]
    for _ in range(10):
        hi0, lo0 = _mulhilo32(0xD2511F53, c0)
        hi1, lo1 = _mulhilo32(0xCD9E8D57, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = (k0 + 0x9E3779B9) & _M32
        k1 = (k1 + 0xBB67AE85) & _M32
    return torch.stack([c0, c1, c2, c3], dim=-1)


def _sample_bits(seed, offset, V):
    """r [B, V] int64: the 23 random bits of every token. Token i uses word
    i & 3 of the Philox block with key (seed lo, seed hi) and counter
    (i >> 2, offset lo, offset hi, 0); int64 seeds and offsets are read as
    two's complement."""
    B = seed.shape[0]
    nblk = (V + 3) // 4
    blk = torch.arange(nblk, device=seed.device).view(1, nblk).expand(B, nblk)
    lo = lambda t: (t & _M32).view(B, 1).expand(B, nblk)
    hi = lambda t: ((t >> 32) & _M32).view(B, 1).expand(B, nblk)
    counter = torch.stack([blk, lo(offset), hi(offset),
                           torch.zeros_like(blk)], dim=-1)
    key = torch.stack([lo(seed), hi(seed)], dim=-1)
    words = philox4x32_10(counter, key)            # [B, nblk, 4]
    return words.reshape(B, nblk * 4)[:, :V] >> 9


def _sample_tokens_ref(logits, temperature, top_k, top_p, seed, offset,
                       details=False):
    """The float64 composition that defines sample_tokens (see there); pure
    tensor ops on the logits' device, no host read. details=True also
    returns (kept [B, V] bool, score [B, V] float64) of the sampled rows:
    rows that are greedy, hold a +inf or nothing above -inf are decided by
    arg-max alone and have kept all False."""
    B, V = logits.shape
    x = logits.double()
    ninf = float("-inf")
    x = torch.where(x.isnan(), torch.full_like(x, ninf), x)
    T = temperature.double().view(B, 1)
    xmax = x.max(dim=1, keepdim=True).values
    first_max = (x == xmax).to(torch.uint8).argmax(dim=1)
    sampled = (T > 0) & (xmax > ninf) & (xmax < float("inf"))
    Ts = torch.where(sampled, T, torch.ones_like(T))
    # top-k: keep what is >= the k-th largest value (ties all stay)
    k = top_k.long().view(B, 1)
    xs, order = x.sort(dim=1, descending=True, stable=True)
    kth = xs.gather(1, (k - 1).clamp(0, V - 1))
    kept = torch.where((k > 0) & (k < V), x >= kth, torch.ones_like(x) > 0)
    # weights of the kept tokens; top-p on the mass strictly above a token
    d = torch.where(sampled, x - xmax, torch.zeros_like(x))
    w = torch.where(kept, torch.exp(d / Ts), torch.zeros_like(x))
    Z = w.sum(dim=1, keepdim=True)
    ws = w.gather(1, order)
    before = ws.cumsum(dim=1) - ws                 # mass ahead in sort order
    run_start = torch.ones_like(xs, dtype=torch.bool)
    run_start[:, 1:] = xs[:, 1:] != xs[:, :-1]
    above_s = torch.where(run_start, before,
                          torch.zeros_like(before)).cummax(dim=1).values
    above = torch.empty_like(above_s).scatter_(1, order, above_s)
    p = top_p.double().view(B, 1)
    stays = (above < p * Z) | (x == xmax)
    kept = kept & torch.where(p < 1, stays, torch.ones_like(stays))
    # exponential race among the kept tokens
    r = _sample_bits(seed, offset, V)
    v = (r.double() + 0.5) * 2.0 ** -23
    E = -torch.log1p(-v)
    score = torch.where(sampled, x, torch.zeros_like(x)) / Ts - torch.log(E)
    score = torch.where(kept, score, torch.full_like(score, ninf))
    smax = score.max(dim=1, keepdim=True).values
    drawn = (score == smax).to(torch.uint8).argmax(dim=1)
    token = torch.where(sampled.view(B), drawn, first_max)
    token = torch.where(xmax.view(B) > ninf, token, torch.zeros_like(token))
    if details:
        kept = kept & sampled
        return token, kept, torch.where(kept, score,
                                        torch.full_like(score, ninf))
    return token


def _sampler_kernel_ok(logits):
    """What the kernel takes; everything else runs the reference."""
    B, V = logits.shape
    return (logits.is_cuda and logits.dtype == torch.bfloat16
            and 1 <= V <= SAMPLER_MAX_VOCAB
            and (V == 1 or logits.stride(1) == 1)
            and logits.data_ptr() % 16 == 0
            and (B <= 1 or (logits.stride(0) >= 0
                            and logits.stride(0) % 8 == 0)))


def sample_tokens(logits, temperature, top_k, top_p, seed, offset):
    """One token per row of logits [B, V] -> int64 [B], each row with its
    own temperature [B] fp32, top_k [B] int32, top_p [B] fp32, seed [B]
    int64 and offset [B] int64, all on the logits' device: nothing is read
    on the host, the call makes no sync and can be captured in a graph.

    Per row, from the logits as given:
      1. NaN counts as -inf; a row with nothing above -inf returns 0. The
         result is always in [0, V).
      2. temperature == 0 (or anything not > 0) is greedy: the lowest index
         of the maximum; the other parameters are ignored. A row that holds
         +inf is decided the same way.
      3. 0 < top_k < V keeps the logits >= the k-th largest value (ties at
         the boundary all stay); top_k == 0 is off.
      4. w_i = exp((x_i - max) / T) over the kept logits, Z = sum(w).
      5. top_p < 1 keeps token i iff sum(w_j : x_j > x_i) < top_p * Z; the
         maximum always stays, equal logits stay or go together.
      6. The draw is an exponential race with noise that depends only on
         (seed, offset, i): Philox4x32-10, key (seed lo, seed hi), counter
         (i >> 2, offset lo, offset hi, 0), token i uses word i & 3;
         r = word >> 9, v = (r + 0.5) * 2^-23, E = -log1p(-v),
         score_i = x_i / T - log(E). The result is the lowest index of the
         maximum score among the kept tokens.
    A row's result depends on nothing but the row and its parameters.

    bf16 GPU logits with V <= 262144 and 16-byte aligned rows run the HIP
    kernel (fp32 scores, bit-identical run to run); the CPU and every other
    input run the same rules as a float64 torch composition, which is the
    reference. Arguments are checked by shape, dtype and device only."""
    if logits.dim() != 2 or logits.shape[1] < 1:
        raise ValueError("logits must be [B, V] with V >= 1")
    if not logits.is_floating_point():
        raise ValueError("logits must be a floating-point tensor")
    _no_grad_inputs("sample_tokens", logits)
    B = logits.shape[0]
    for name, t, dt in (("temperature", temperature, torch.float32),
                        ("top_k", top_k, torch.int32),
                        ("top_p", top_p, torch.float32),
                        ("seed", seed, torch.int64),
                        ("offset", offset, torch.int64)):
        if not torch.is_tensor(t) or t.dtype != dt \
                or tuple(t.shape) != (B,) or t.device != logits.device:
            raise ValueError(f"{name} must be [B] {dt} on the logits' device")
    if B == 0:
        return torch.empty(0, dtype=torch.long, device=logits.device)
    if _sampler_kernel_ok(logits):
        return _ext().sample_tokens(logits, temperature.contiguous(),
                                    top_k.contiguous(), top_p.contiguous(),
                                    seed.contiguous(), offset.contiguous())
    return _sample_tokens_ref(logits, temperature, top_k, top_p, seed, offset)


# ---------------------------------------------------------------------------
# Per-token log-probabilities (serving): what the sampler's pick was worth.
# Inference-only, no autograd, no host sync on the GPU.
# ---------------------------------------------------------------------------
LOGPROBS_MAX_TOP = 32


def _token_logprobs_ref(logits, token, temperature, top_n=0,
                        dtype=torch.float32):
    """The float64 composition that defines token_logprobs (see there); pure
    tensor ops on the logits' device. On the GPU nothing is read on the
    host and a token outside [0, V) gives the sentinels; on the CPU it is a
    ValueError. dtype=torch.float64 returns the log-probs unrounded."""
    B, V = logits.shape
    inf = float("inf")
    x = logits.double()
    x = torch.where(x.isnan(), torch.full_like(x, -inf), x)
    T = temperature.double().view(B, 1)
    T = torch.where(T > 0, T, torch.ones_like(T))
    xmax = x.max(dim=1, keepdim=True).values
    has_pinf = xmax == inf
    nothing = xmax == -inf
    edge = has_pinf | nothing
    a = torch.where(edge, torch.zeros_like(x), x - xmax) / T
    lp = a - torch.log(torch.exp(a).sum(dim=1, keepdim=True))
    # a row holding +inf: its +inf entries share the mass
    n_pinf = (x == inf).sum(dim=1, keepdim=True).double()
    lp_pinf = torch.where(x == inf, -torch.log(n_pinf),
                          torch.full_like(x, -inf))
    lp = torch.where(has_pinf, lp_pinf, lp)
    # a row with nothing above -inf has no distribution
    lp = torch.where(nothing, torch.full_like(x, float("nan")), lp)
    tok = token.view(B, 1)
    ok = (tok >= 0) & (tok < V)
    if not logits.is_cuda and not bool(ok.all()):
        raise ValueError(f"token must be in [0, {V})")
    tc = tok.clamp(0, V - 1)
    logprob = torch.where(ok, lp.gather(1, tc),
                          torch.full_like(xmax, float("nan")))
    above = (x > x.gather(1, tc)).sum(dim=1, keepdim=True)
    rank = torch.where(ok, above + 1, torch.zeros_like(above))
    n = min(top_n, V)
    top_ids = torch.full((B, top_n), -1, dtype=torch.int32,
                         device=logits.device)
    top_lp = torch.full((B, top_n), -inf, dtype=dtype, device=logits.device)
    if n > 0:
        # stable: equal logits keep index order, the lowest index first
        order = x.sort(dim=1, descending=True, stable=True).indices[:, :n]
        top_ids[:, :n] = order
        top_lp[:, :n] = lp.gather(1, order)
    return (logprob.view(B).to(dtype), rank.view(B).to(torch.int32), top_ids,
            top_lp)


def token_logprobs(logits, token, temperature, top_n=0):
    """For every row of logits [B, V], the log-probability and rank of
    token [B] int64 under temperature [B] fp32 (both on the logits' device)
    and the top_n most likely tokens: (logprob [B] fp32, rank [B] int32,
    top_ids [B, top_n] int32, top_logprobs [B, top_n] fp32). top_n is a host
    int in [0, 32]; nothing is read on the host, the call makes no sync and
    can be captured in a graph.

    Per row, from the logits as given:
      1. NaN counts as -inf. T_eff = T if T > 0 else 1: a greedy row
         reports the raw distribution.
      2. a_i = (x_i - max) / T_eff and logprob = a_tok - log(sum_j exp(a_j))
         over the whole vocabulary. The sampler's top-k and top-p filters
         are NOT applied: with the filters off this is exactly the
         distribution the token was drawn from, with them on it is the
         distribution before filtering.
      3. rank = 1 + #{j : x_j > x_tok}.
      4. top_ids are the top_n largest logits, descending, equal logits by
         the lowest index first; top_logprobs are their log-probs at the
         same T_eff. Slots past V hold id -1 and -inf.
      5. A row holding +inf: its +inf entries get -log(their count), all
         others -inf. A row with nothing above -inf: log-probs are NaN,
         the ids are the lowest indices.
      6. A token outside [0, V): on the GPU logprob NaN and rank 0, and
         nothing is read outside the row; on the CPU a ValueError.
    A row's result depends on nothing but the row and its own parameters.

    Dispatch is sample_tokens': bf16 GPU logits with V <= 262144 and 16-byte
    aligned rows run the HIP kernel (fp32 terms summed in fp64 by a fixed
    tree, bit-identical run to run, for any B and row position); the CPU and
    every other input run the same rules as a float64 torch composition,
    which is the reference. Arguments are checked by shape, dtype and device
    only."""
    if logits.dim() != 2 or logits.shape[1] < 1:
        raise ValueError("logits must be [B, V] with V >= 1")
    if not logits.is_floating_point():
        raise ValueError("logits must be a floating-point tensor")
    _no_grad_inputs("token_logprobs", logits)
    if not isinstance(top_n, int) or isinstance(top_n, bool) \
            or not 0 <= top_n <= LOGPROBS_MAX_TOP:
        raise ValueError(
            f"top_n must be an int in [0, {LOGPROBS_MAX_TOP}], got {top_n!r}")
    B = logits.shape[0]
    for name, t, dt in (("token", token, torch.int64),
                        ("temperature", temperature, torch.float32)):
        if not torch.is_tensor(t) or t.dtype != dt \
                or tuple(t.shape) != (B,) or t.device != logits.device:
            raise ValueError(f"{name} must be [B] {dt} on the logits' device")
    if B == 0:
        dev = logits.device
        return (torch.empty(0, dtype=torch.float32, device=dev),
                torch.empty(0, dtype=torch.int32, device=dev),
                torch.empty(0, top_n, dtype=torch.int32, device=dev),
                torch.empty(0, top_n, dtype=torch.float32, device=dev))
    if _sampler_kernel_ok(logits):
        return tuple(_ext().token_logprobs(logits, token.contiguous(),
                                           temperature.contiguous(), top_n))
    return _token_logprobs_ref(logits, token, temperature, top_n)


# ---------------------------------------------------------------------------
# Multi-tensor pack/unpack (GPU data plane: packed state-dict transfers)
# ---------------------------------------------------------------------------
PACK_ALIGN = 16  # bytes; segment starts in the flat buffer are 16B-aligned


def aligned_offsets(numels, elem_size):
    """Element offsets into the packed flat buffer with every segment start
    16B-aligned (so the pack kernel runs pure uint4 copies). Returns
    (offsets, total_elems)."""
    step = PACK_ALIGN // elem_size
    offs, cur = [], 0
    for n in numels:
        offs.append(cur)
        cur += -(-n // step) * step  # round numel up to the alignment step
    return offs, cur


def _all_aligned(tensors):
    """The pack kernel copies 16 B vectors from each tensor's data pointer.
    A contiguous view into the middle of an allocation (t[1:]) need not
    start on such a boundary; calls holding one take the per-tensor copy."""
    return all(t.data_ptr() % PACK_ALIGN == 0 for t in tensors)


def pack_tensors(tensors, flat=None):
    """Pack same-dtype contiguous GPU tensors into one flat buffer with a
    single kernel (vs torch.cat's per-tensor copies). Returns (flat,
    offsets) where offsets are element positions (aligned)."""
    dt = tensors[0].dtype
    es = dt.itemsize
    numels = [t.numel() for t in tensors]
    offs, total = aligned_offsets(numels, es)
    dev = tensors[0].device
    if flat is None:
        flat = torch.zeros(total, dtype=dt, device=dev)
    if (dev.type == "cuda" and hip_available()
            and _all_aligned(list(tensors) + [flat])):
        ptrs = torch.tensor([t.data_ptr() for t in tensors],
                            dtype=torch.int64).to(dev, non_blocking=True)
        nb = torch.tensor([n * es for n in numels],
                          dtype=torch.int64).to(dev, non_blocking=True)
        ob = torch.tensor([o * es for o in offs],
                          dtype=torch.int64).to(dev, non_blocking=True)
        _ext().pack_segments(flat, ptrs, nb, ob, True, max(numels) * es)
    else:
        for t, o, n in zip(tensors, offs, numels):
            flat[o:o + n].copy_(t.reshape(-1))
    return flat, offs


def unpack_tensors(flat, tensors, offsets=None):
    """Scatter a packed flat buffer back into pre-allocated tensors (the
    inverse of pack_tensors) with one kernel on GPU."""
    es = flat.dtype.itemsize
    numels = [t.numel() for t in tensors]
    if offsets is None:
        offsets, _ = aligned_offsets(numels, es)
    if (flat.is_cuda and hip_available()
            and all(t.is_contiguous() for t in tensors)
            and all(o * es % PACK_ALIGN == 0 for o in offsets)
            and _all_aligned(list(tensors) + [flat])):
        dev = flat.device
        ptrs = torch.tensor([t.data_ptr() for t in tensors],
                            dtype=torch.int64).to(dev, non_blocking=True)
        nb = torch.tensor([n * es for n in numels],
                          dtype=torch.int64).to(dev, non_blocking=True)
        ob = torch.tensor([o * es for o in offsets],
                          dtype=torch.int64).to(dev, non_blocking=True)
        _ext().pack_segments(flat, ptrs, nb, ob, False, max(numels) * es)
    else:
        for t, o in zip(tensors, offsets):
            t.copy_(flat[o:o + t.numel()].view(t.shape))
    return tensors


# ---------------------------------------------------------------------------
# bf16 transposes + bias-free linear with K-contiguous backward operands
# ---------------------------------------------------------------------------
def kcontig_enabled():
    """KT_KCONTIG=0 turns the K-contiguous backward off everywhere (engine
    shadows and the wgrad layout table), so one tree can run an A/B."""
    return os.environ.get("KT_KCONTIG", "1") != "0"


def _transpose_kernel_ok(src):
    return (src.is_cuda and src.dtype == torch.bfloat16 and src.dim() == 2
            and src.shape[0] > 0 and src.shape[1] > 0
            and src.shape[0] % 8 == 0 and src.shape[1] % 8 == 0
            and src.stride(1) == 1 and src.stride(0) >= src.shape[1]
            and src.stride(0) % 8 == 0 and src.data_ptr() % 16 == 0)


def transpose_bf16(src):
    """dst[C, R] = src[R, C].t(), contiguous. bf16 GPU matrices whose dims
    (and row stride) are multiples of 8 run the LDS-tiled HIP kernel;
    anything else, and CPU, is .t().contiguous()."""
    if _transpose_kernel_ok(src):
        return _ext().transpose_bf16(src)
    return src.t().contiguous()


def transpose_table(segments, src_numel, dst_numel, device):
    """Device-side segment table for transpose_segments_bf16, built once.

    segments: (src_offset, dst_offset, rows, cols) in elements. Every
    segment is checked on the host against both buffers (the kernel trusts
    the table). Returns (table int64 [nseg, 4], max_tiles)."""
    max_tiles = 0
    spans = []
    for so, do, r, c in segments:
        if min(so, do) < 0 or r <= 0 or c <= 0 or r % 8 or c % 8 \
                or so % 8 or do % 8:
            raise ValueError(f"segment {(so, do, r, c)}: offsets, rows and "
                             "cols must be multiples of 8")
        if so + r * c > src_numel or do + r * c > dst_numel:
            raise ValueError(f"segment {(so, do, r, c)} is out of bounds")
        spans.append((do, do + r * c))
        max_tiles = max(max_tiles, -(-r // 64) * -(-c // 64))
    spans.sort()
    for (_, e0), (s1, _) in zip(spans, spans[1:]):
        if s1 < e0:
            raise ValueError("destination segments overlap")
    table = torch.tensor([list(s) for s in segments], dtype=torch.int64)
    return table.reshape(-1, 4).to(device), max_tiles


def transpose_segments_bf16(flat_src, flat_dst, table, max_tiles):
    """flat_dst[do : do + r*c] = flat_src[so : so + r*c].view(r, c).t() for
    every row of `table` (see transpose_table), in one launch on GPU."""
    if flat_src.is_cuda:
        _ext().transpose_segments_bf16(flat_src, flat_dst, table, max_tiles)
        return
    for so, do, r, c in table.tolist():
        flat_dst[do:do + r * c].view(c, r).copy_(
            flat_src[so:so + r * c].view(r, c).t())


class ShadowClock:
    """Write counter of the storage a weight lives in (one per optimizer
    bucket). Whoever writes the weights outside autograd's view bumps it
    BEFORE the write; a shadow is fresh only while its stamp matches."""
    __slots__ = ("value",)

    def __init__(self):
        self.value = (0, 0)  # (engine step count, other-writer counter)


def stamp_weight_t(weight_t, weight, clock=None):
    """Mark weight_t as holding weight.t() as of now."""
    weight_t._kt_stamp = (weight._version, clock,
                          clock.value if clock is not None else None)
    return weight_t


def make_weight_t(weight, clock=None):
    """A stamped [in, out] shadow of a [out, in] weight."""
    with torch.no_grad():
        wt = transpose_bf16(weight.detach())
    return stamp_weight_t(wt, weight, clock)


def weight_t_is_fresh(weight_t, weight):
    """True only when weight_t was stamped against this weight's current
    version and its bucket has not been written since. An unstamped or
    mismatched shadow is never used."""
    stamp = getattr(weight_t, "_kt_stamp", None)
    if stamp is None or weight_t.shape != (weight.shape[1], weight.shape[0]):
        return False
    version, clock, value = stamp
    if version != weight._version:
        return False
    return clock is None or clock.value == value


# wgrad operand layouts for dW[out, in] = dY[T, out]^T @ X[T, in]:
#   "a"  dY.t() @ X             neither operand K(=T)-contiguous
#   "b"  dY.t() @ (X^T).t()     X^T materialised by transpose_bf16
#   "c"  (dY^T) @ X             dY^T materialised
#   "d"  (dY^T) @ (X^T).t()     both
# Keyed by (in, out); a layer class is listed only where its GEMM plus
# transpose time beat "a" in tests/bench_gemm_layouts.py on MI355X
# (profiles/kcontig_backward.md). Everything else keeps "a".
WGRAD_VARIANTS = ("a", "b", "c", "d")
WGRAD_LAYOUT = {
    (4096, 4096): "b",     # wo:        0.47 -> 0.44 ms at T=16384
    (4096, 28672): "b",    # w_gate_up: 3.21 -> 2.82 ms
    (14336, 4096): "c",    # w_down:    1.94 -> 1.81 ms
    (4096, 128256): "b",   # lm_head:  14.74 -> 12.92 ms
}


def _wgrad(dy2, x2, variant):
    if variant == "b":
        return dy2.t() @ transpose_bf16(x2).t()
    if variant == "c":
        return transpose_bf16(dy2) @ x2
    if variant == "d":
        return transpose_bf16(dy2) @ transpose_bf16(x2).t()
    return dy2.t() @ x2


class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, weight_t, wgrad):
        ctx.save_for_backward(x, weight)
        # not a saved tensor: the engine refreshes the shadow in place
        # between steps, and freshness is judged by its stamp in backward
        ctx.weight_t = weight_t
        ctx.wgrad = wgrad
        return torch.nn.functional.linear(x, weight)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        out_f, in_f = weight.shape
        dy2 = dy.reshape(-1, out_f)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            wt = ctx.weight_t
            if wt is not None and weight_t_is_fresh(wt, weight):
                dx = dy2 @ wt.t()      # both operands K(=out)-contiguous
            else:
                dx = dy2 @ weight
            dx = dx.view(x.shape)
        if ctx.needs_input_grad[1]:
            variant = ctx.wgrad
            if variant is None:
                variant = (WGRAD_LAYOUT.get((in_f, out_f), "a")
                           if kcontig_enabled() and dy2.is_cuda else "a")
            dw = _wgrad(dy2, x.reshape(-1, in_f), variant)
        return dx, dw, None, None


def linear(x, weight, weight_t=None, wgrad=None):
    """Bias-free y = x @ weight.t() whose backward feeds hipBLASLt
    K-contiguous operands where that is faster.

    weight_t: optional stamped [in, out] shadow of weight (make_weight_t /
    stamp_weight_t). dX = dY @ weight_t.t() when it is fresh, else
    dY @ weight. wgrad: force one of WGRAD_VARIANTS (None = WGRAD_LAYOUT).
    Without grad this is plain F.linear."""
    if wgrad is not None and wgrad not in WGRAD_VARIANTS:
        raise ValueError(f"wgrad must be one of {WGRAD_VARIANTS}")
    if not torch.is_grad_enabled() or not (x.requires_grad
                                           or weight.requires_grad):
        return torch.nn.functional.linear(x, weight)
    return _LinearFn.apply(x, weight, weight_t, wgrad)


class Linear(torch.nn.Linear):
    """nn.Linear (bias=False only) routed through ops.linear. Parameter and
    state-dict names are nn.Linear's. weight_t is a plain attribute (not a
    parameter, not a buffer): FlatDDP installs and refreshes it."""

    def __init__(self, in_features, out_features, bias=False, device=None,
                 dtype=None):
        if bias:
            raise ValueError("ops.Linear is bias-free")
        super().__init__(in_features, out_features, bias=False, device=device,
                         dtype=dtype)
        self.weight_t = None

    def _apply(self, fn, recurse=True):
        # .to()/.cuda()/.half() give the weight new storage: drop the shadow
        self.weight_t = None
        return super()._apply(fn, recurse)

    def forward(self, x):
        return linear(x, self.weight, self.weight_t)


# ---------------------------------------------------------------------------
# FP8 weight-only linear (W8A16, serving decode). Inference-only.
#
# Format: weight_q [out, in] torch.float8_e4m3fn (OCP e4m3), row-major like
# nn.Linear.weight, and one static fp32 scale per output row that is a power
# of two: scale[n] = 2^ceil(log2(amax_n / 448)). The represented matrix is
# Wq = float(weight_q) * scale[:, None]; with a power-of-two scale every
# element of Wq is exactly a bf16 value, so the kernel, the composition below
# and a plain bf16 model holding Wq all multiply by the same matrix and
# differ in accumulation order only.
# ---------------------------------------------------------------------------
W8_DTYPE = torch.float8_e4m3fn
W8_MAX = 448.0
W8_SCALE_EXP = 40          # scales lie in [2^-40, 2^40]
W8_MAX_ROWS = 32           # the kernel's M; more rows run the composition
W8_K_MULTIPLE = 128


def _check_w8_scale_values(scale):
    """Host check of scale values (a device tensor is copied over, which
    syncs: call this at construction, not per step)."""
    s = scale.detach().to("cpu", torch.float32)
    mant, exp = torch.frexp(s)
    ok = s.isfinite() & (s > 0) & (mant == 0.5) \
        & (exp - 1 >= -W8_SCALE_EXP) & (exp - 1 <= W8_SCALE_EXP)
    if not bool(ok.all()):
        raise ValueError("weight_scale must be finite, positive powers of "
                         f"two in [2^-{W8_SCALE_EXP}, 2^{W8_SCALE_EXP}]")


def _check_w8(weight_q, weight_scale):
    """Dtype, shape and device of a quantised weight; the scale values only
    where looking is no device sync (on the CPU)."""
    if not torch.is_tensor(weight_q) or weight_q.dtype != W8_DTYPE:
        raise ValueError("weight_q must be torch.float8_e4m3fn, got "
                         f"{getattr(weight_q, 'dtype', type(weight_q))}")
    if weight_q.dim() != 2:
        raise ValueError("weight_q must be [out_features, in_features]")
    if not torch.is_tensor(weight_scale) \
            or weight_scale.dtype != torch.float32:
        raise ValueError("weight_scale must be fp32")
    if tuple(weight_scale.shape) != (weight_q.shape[0],):
        raise ValueError("weight_scale must be [out_features], got "
                         f"{tuple(weight_scale.shape)}")
    if weight_scale.device != weight_q.device:
        raise ValueError("weight_q and weight_scale must be on one device")
    if not weight_scale.is_cuda:
        _check_w8_scale_values(weight_scale)


def quantize_weight_fp8(w):
    """[out, in] floating-point weight -> (weight_q e4m3, weight_scale fp32).

    scale[n] is the smallest power of two with amax_n / scale[n] <= 448
    (2^ceil(log2(amax_n / 448)), computed exactly from the exponent of
    amax_n, clamped to [2^-40, 2^40]); an all-zero row gets 1.0. Then
    q = (w.float() * (1 / scale)[:, None]).clamp(-448, 448).to(e4m3): the
    multiply is exact, the conversion rounds to nearest even. The row maxima
    of |q| land in (224, 448]; no NaN byte is produced."""
    if not torch.is_tensor(w) or w.dim() != 2 or not w.is_floating_point() \
            or w.dtype in _FLOAT8_DTYPES:
        raise ValueError("w must be a 2-D floating-point weight [out, in]")
    wf = w.detach().float()
    amax = wf.abs().amax(dim=1) if wf.shape[1] else wf.new_zeros(wf.shape[0])
    if not bool(amax.isfinite().all()):
        raise ValueError("w holds NaN or inf")
    # amax = m * 2^e with m in [0.5, 1) and 448 = 0.875 * 2^9, so
    # amax <= 448 * 2^p  <=>  p >= e - 9 (m <= 0.875) or e - 8 (m > 0.875)
    mant, exp = torch.frexp(amax)
    p = exp - 9 + (mant > 0.875).to(exp.dtype)
    p = p.clamp(-W8_SCALE_EXP, W8_SCALE_EXP)
    scale = torch.ldexp(torch.ones_like(amax), p)
    scale = torch.where(amax == 0, torch.ones_like(scale), scale)
    q = (wf * scale.reciprocal()[:, None]).clamp(-W8_MAX, W8_MAX).to(W8_DTYPE)
    return q, scale


def dequantize_weight_fp8(weight_q, weight_scale, dtype=torch.bfloat16):
    """Wq = float(weight_q) * weight_scale[:, None] as `dtype`: exact in
    bf16, fp32 and fp64 (e4m3 has at most 4 significant bits and the scale
    only shifts the exponent), rounded once for any other dtype."""
    _check_w8(weight_q, weight_scale)
    if dtype in (torch.bfloat16, torch.float32, torch.float64):
        # one temporary of the result's size; the product is exact
        return weight_q.to(dtype).mul_(weight_scale.to(dtype)[:, None])
    return (weight_q.float() * weight_scale[:, None]).to(dtype)


def _w8_rows(x, K):
    """x [..., K] as a 2-D [M, K] view, or None where that needs a copy."""
    if x.dim() == 2:
        return x
    try:
        return x.view(-1, K)
    except RuntimeError:
        return None


def _linear_w8_kernel_ok(x, weight_q, weight_scale):
    """What the kernel takes; everything else runs the composition."""
    K = weight_q.shape[1]
    if not (x.is_cuda and x.dtype == torch.bfloat16 and K >= W8_K_MULTIPLE
            and K % W8_K_MULTIPLE == 0 and K <= 1 << 24
            and 1 <= weight_q.shape[0] <= 1 << 30
            and weight_q.is_contiguous()):
        return False
    x2 = _w8_rows(x, K)
    if x2 is None:
        return False
    M = x2.shape[0]
    return (1 <= M <= W8_MAX_ROWS and x2.stride(1) == 1
            and x2.data_ptr() % 16 == 0
            and (M == 1 or (0 <= x2.stride(0) <= 1 << 24
                            and x2.stride(0) % 8 == 0)))


def linear_w8_splits(out_features, in_features):
    """The split-K factor the kernel chooses for an [out, in] weight: a
    function of the shape alone, never of the batch or of device data."""
    return int(_ext().linear_w8_splits(out_features, in_features))


def linear_w8(x, weight_q, weight_scale, num_splits=None):
    """y[..., n] = round_to_x_dtype(sum_k float(x[..., k]) * Wq[n, k]) with
    Wq = float(weight_q) * weight_scale[:, None] (quantize_weight_fp8):
    fp32 accumulation in an order the implementation chooses, one rounding
    at the end. x is [..., K]; the leading dimensions flatten to M rows.
    Inference-only: x must not require grad while grad is enabled.

    bf16 GPU x with 1 <= M <= 32, K % 128 == 0, a contiguous last dim,
    16-byte aligned rows and a contiguous weight_q runs the gfx950 kernel
    (weights streamed once as fp8, bit-identical run to run, a row's result
    independent of the other rows in the call). Any other valid input, the
    CPU included, runs F.linear(x, dequantize_weight_fp8(q, scale, x.dtype)),
    whose temporary comes from the caching allocator. num_splits overrides
    the kernel's split-K factor (tests); the composition ignores it.

    Wrong dtypes (weight_q not float8_e4m3fn, weight_scale not fp32), wrong
    shapes and mismatched devices raise. Scale values are checked on the CPU
    only (LinearW8 checks them once at construction)."""
    _check_w8(weight_q, weight_scale)
    if not torch.is_tensor(x) or not x.is_floating_point() \
            or x.dtype in _FLOAT8_DTYPES:
        raise ValueError("x must be a floating-point tensor")
    N, K = weight_q.shape
    if x.dim() < 1 or x.shape[-1] != K:
        raise ValueError(f"x must be [..., {K}], got {tuple(x.shape)}")
    if x.device != weight_q.device:
        raise ValueError(f"x is on {x.device}, the weight on "
                         f"{weight_q.device}")
    if num_splits is not None and not 1 <= int(num_splits) <= 64:
        raise ValueError("num_splits must be in [1, 64]")
    if torch.is_grad_enabled() and x.requires_grad:
        raise RuntimeError("linear_w8 is inference-only: x requires grad")
    if _linear_w8_kernel_ok(x, weight_q, weight_scale):
        y = _ext().linear_w8(_w8_rows(x, K), weight_q,
                             weight_scale.contiguous(), int(num_splits or 0))
        return y.view(*x.shape[:-1], N)
    return torch.nn.functional.linear(
        x, dequantize_weight_fp8(weight_q, weight_scale, x.dtype))


class LinearW8(torch.nn.Module):
    """Bias-free linear layer with FP8 weights (ops.linear_w8). weight_q
    [out, in] e4m3 and weight_scale [out] fp32 are buffers: state_dict,
    load_state_dict and .to(device) carry them; a dtype cast of the model
    (.to(torch.bfloat16), .half()) leaves them as they are."""

    def __init__(self, in_features, out_features, device=None):
        super().__init__()
        self.in_features = in_features
        self.out_features = out_features
        self.register_buffer("weight_q", torch.zeros(
            out_features, in_features, dtype=W8_DTYPE, device=device))
        self.register_buffer("weight_scale", torch.ones(
            out_features, dtype=torch.float32, device=device))

    @classmethod
    def from_quantized(cls, weight_q, weight_scale):
        """Wrap an existing (weight_q, weight_scale) pair; the scale values
        are validated on the host here, once."""
        _check_w8(weight_q, weight_scale)
        _check_w8_scale_values(weight_scale)
        mod = cls(weight_q.shape[1], weight_q.shape[0], device="meta")
        mod.weight_q = weight_q.contiguous()
        mod.weight_scale = weight_scale.contiguous()
        return mod

    @classmethod
    def from_linear(cls, lin):
        """Quantise an nn.Linear (ops.Linear included) without bias."""
        if not isinstance(lin, torch.nn.Linear):
            raise TypeError(f"expected nn.Linear, got {type(lin).__name__}")
        if lin.bias is not None:
            raise ValueError("LinearW8 is bias-free: the layer has a bias")
        return cls.from_quantized(*quantize_weight_fp8(lin.weight))

    def _apply(self, fn, recurse=True):
        # device moves apply; dtype casts must not touch the fp8 bytes or
        # round the scale
        q, s = self.weight_q, self.weight_scale
        super()._apply(fn, recurse)
        if self.weight_q.dtype != W8_DTYPE:
            self.weight_q = q.to(self.weight_q.device)
        if self.weight_scale.dtype != torch.float32:
            self.weight_scale = s.to(self.weight_scale.device)
        return self

    def forward(self, x):
        return linear_w8(x, self.weight_q, self.weight_scale)

    def extra_repr(self):
        return (f"in_features={self.in_features}, "
                f"out_features={self.out_features}, weight=e4m3")


# ---------------------------------------------------------------------------
# Fused AdamW on flat bf16 buckets (used by kubetorch_amd.parallel)
# ---------------------------------------------------------------------------
def adamw_(p, g, m, v, lr, beta1, beta2, eps, wd, step, grad_scale=1.0):
    if p.is_cuda:
        _ext().adamw_(p, g, m, v, lr, beta1, beta2, eps, wd, step, grad_scale)
        return
    # CPU reference (fp32 math, bf16 params)
    gf = g.float() * grad_scale
    pf = p.float()
    m.mul_(beta1).add_(gf, alpha=1 - beta1)
    v.mul_(beta2).addcmul_(gf, gf, value=1 - beta2)
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    mhat = m / bc1
    vhat = v / bc2
    pf = pf - lr * (mhat / (vhat.sqrt() + eps) + wd * pf)
    p.copy_(pf.to(p.dtype))
