"""Edge-shape, high-precision tests for the fused HIP ops.

tests/test_ops.py checks each kernel at one friendly shape with loose
tolerances. The cases here run the code paths that training takes and
that file does not reach: grid-strides, second loop iterations, tails,
strided views, masked logits, slices of a flat bucket. They compare with
plain float64 PyTorch references computed from the same bf16 inputs,
under a one-bf16-ulp rule (assert_bf16_ulp).

Every case is a `_check(device, ...)` run twice: on "cpu" against the
project's fp32 reference path (this proves the test and its tolerance on
any machine) and on "cuda" under the gpu marker. Cases that call
ops._ext() directly are GPU-only.

Lines starting with "[edges]" report the measured error of every fp32
output bound; run with -s to see them.
"""
import math

import pytest
import torch

from kubetorch_amd import ops

BF16 = torch.bfloat16
F64 = torch.float64
EPS = 1e-5
EPS32 = float(torch.tensor(EPS, dtype=torch.float32))  # what the kernel gets


def _f64(t):
    return t.detach().to(F64)


def _f32exact(v):
    """A Python float rounded to fp32, as the launchers receive it."""
    return float(torch.tensor(v, dtype=torch.float32))


def _bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8).cpu()


def _note(name, value):
    print(f"[edges] {name} {value:.3e}")


def _both(name, check, cases=None):
    """Register test_<name>_cpu (unmarked) and test_<name>_gpu (gpu)."""
    if cases is None:
        def cpu():
            check("cpu")

        def gpu():
            check("cuda")
    else:
        ids = ["-".join(str(v) for v in c) for c in cases]

        def cpu(case):
            check("cpu", *case)

        def gpu(case):
            check("cuda", *case)
        par = pytest.mark.parametrize("case", cases, ids=ids)
        cpu, gpu = par(cpu), par(gpu)
    gpu = pytest.mark.gpu(gpu)
    for fn, suffix in ((cpu, "cpu"), (gpu, "gpu")):
        fn.__name__ = fn.__qualname__ = f"test_{name}_{suffix}"
        globals()[fn.__name__] = fn


# ---------------------------------------------------------------------------
# The comparison rule
# ---------------------------------------------------------------------------
def assert_bf16_ulp(actual, ref64, extra_abs=0, floor=1e-30, msg=""):
    """bf16 result against a float64 reference.

    Hard bound, every element: |a - ref| <= 2**-7*|ref| + extra_abs + floor.
    That is one bf16 ulp: half an ulp of output rounding plus a flip at a
    rounding boundary caused by fp32 ordering.
    Cap: at most 0.1 % of the elements exceed half an ulp,
    2**-8*|ref|*(1 + 2**-10) + extra_abs + floor.
    NaN and inf positions must match the reference exactly. `floor` excuses
    flush-to-zero of results below 1e-30 and nothing else; `extra_abs` is
    the op's fp32 accumulation term (a tensor or a number), derived where
    it is used.
    """
    a = _f64(actual).cpu()
    r = _f64(ref64).cpu()
    assert a.shape == r.shape, f"{msg}: shape {tuple(a.shape)} vs {tuple(r.shape)}"
    e = extra_abs
    if torch.is_tensor(e):
        e = _f64(e).cpu().expand_as(r)
    else:
        e = torch.full_like(r, float(e))
    assert torch.equal(a.isnan(), r.isnan()), f"{msg}: NaN positions differ"
    inf = r.isinf()
    assert torch.equal(a.isinf(), inf), f"{msg}: inf positions differ"
    assert torch.equal(a[inf], r[inf]), f"{msg}: inf signs differ"
    fin = r.isfinite()
    a, r, e = a[fin], r[fin], e[fin]
    err = (a - r).abs()
    hard = 2.0 ** -7 * r.abs() + e + floor
    bad = err > hard
    if bad.any():
        i = int((err - hard).argmax())
        raise AssertionError(
            f"{msg}: {int(bad.sum())} of {err.numel()} elements beyond one "
            f"bf16 ulp; worst got {a[i].item()!r}, reference {r[i].item()!r},"
            f" bound {hard[i].item():.3e}")
    soft = 2.0 ** -8 * r.abs() * (1 + 2.0 ** -10) + e + floor
    over = int((err > soft).sum())
    assert over <= 1e-3 * err.numel(), (
        f"{msg}: {over} of {err.numel()} elements beyond half a bf16 ulp "
        "(cap 0.1 %)")


def _assert_fp32(actual, ref64, rtol=0.0, atol=0.0, msg="", cap=None):
    """fp32 result against float64: |a - ref| <= rtol*|ref| + atol*max(1,
    |ref|), the whole bound held below `cap` where one is given. Prints
    the largest observed error, absolute and as a fraction of its bound."""
    a, r = _f64(actual).cpu(), _f64(ref64).cpu()
    assert a.shape == r.shape, msg
    assert bool(a.isfinite().all()), f"{msg}: non-finite values"
    err = (a - r).abs()
    bound = rtol * r.abs() + atol * r.abs().clamp(min=1.0)
    if cap is not None:
        bound = bound.clamp(max=cap)
    if err.numel():
        _note(msg.replace(" ", "_") + "_max_abs_err", err.max().item())
        _note(msg.replace(" ", "_") + "_max_err_over_bound",
              (err / bound).max().item())
    bad = err > bound
    if bad.any():
        i = int((err / bound).argmax())
        raise AssertionError(
            f"{msg}: worst got {a.reshape(-1)[i].item()!r}, reference "
            f"{r.reshape(-1)[i].item()!r}, error {err.reshape(-1)[i].item():.3e}"
            f" over bound {bound.reshape(-1)[i].item():.3e}")


def test_ulp_rule_catches_wrong_results():
    """The helper itself: exact rounding passes; a dropped term, a 2-ulp
    error, too many 1-ulp errors and a stray NaN do not."""
    torch.manual_seed(0)
    ref = torch.randn(4096, dtype=F64)
    good = ref.to(BF16)
    assert_bf16_ulp(good, ref)
    # the bf16 neighbour on the other side of ref: off by 0.5..1 ulp
    toward = torch.where(good.double().abs() < ref.abs(), 1, -1).to(torch.int16)
    up = (good.view(torch.int16) + toward).view(BF16)
    few = good.clone()
    few[:3] = up[:3]
    assert_bf16_ulp(few, ref)  # 3 of 4096 is under the cap
    with pytest.raises(AssertionError, match="bf16 ulp"):
        assert_bf16_ulp(up, ref)
    many = good.clone()
    many[:64] = up[:64]  # most of 64 in 4096 is over the cap
    with pytest.raises(AssertionError, match="bf16 ulp"):
        assert_bf16_ulp(many, ref)
    four = (good.view(torch.int16) + 4).view(BF16)
    one_bad = good.clone()
    one_bad[100] = four[100]
    with pytest.raises(AssertionError, match="one bf16 ulp"):
        assert_bf16_ulp(one_bad, ref)
    nan = good.clone()
    nan[5] = float("nan")
    with pytest.raises(AssertionError, match="NaN"):
        assert_bf16_ulp(nan, ref)
    with pytest.raises(AssertionError):
        assert_bf16_ulp(torch.zeros(8, dtype=BF16), torch.full((8,), 1e-3, dtype=F64))


# ---------------------------------------------------------------------------
# RMSNorm / AddRMSNorm
# ---------------------------------------------------------------------------
def _ref_rmsnorm64(s, w, dy=None, ds=None):
    """float64 RMSNorm of the bf16 stream `s`, with the fp32 accumulation
    terms of the outputs:
      y:  2**-20*|y|; invrms carries the error of an fp32 sum and rsqrtf
          (the invrms bound below allows 1e-5, this is a tenth of it) and
          y two more fp32 products.
      dx: 2**-20*(|dy*w|*ir + |x|*ir**3*sum_j|dy_j*w_j*x_j|/H), the two
          terms of dx with the sum taken over magnitudes; plus the fp32
          add of ds (2**-23*|ds|) on the fused path.
      dw: 2**-20*sum_rows|dy*x*ir|."""
    H = s.shape[-1]
    s64 = _f64(s).reshape(-1, H)
    w64 = _f64(w)
    ir = (s64.pow(2).mean(-1, keepdim=True) + EPS32).rsqrt()
    out = {"y": s64 * ir * w64, "ir": ir.squeeze(-1)}
    out["y_extra"] = 2.0 ** -20 * out["y"].abs()
    if dy is not None:
        dy64 = _f64(dy).reshape(-1, H)
        t = dy64 * w64 * s64
        S = t.sum(-1, keepdim=True)
        dx = ir * dy64 * w64 - s64 * ir ** 3 * S / H
        ex = 2.0 ** -20 * ((dy64 * w64).abs() * ir + s64.abs() * ir ** 3
                           * t.abs().sum(-1, keepdim=True) / H)
        if ds is not None:
            ds64 = _f64(ds).reshape(-1, H)
            dx = dx + ds64
            ex = ex + 2.0 ** -23 * ds64.abs()
        out["dx"], out["dx_extra"] = dx, ex
        out["dw"] = (dy64 * s64 * ir).sum(0)
        out["dw_extra"] = 2.0 ** -20 * (dy64 * s64 * ir).abs().sum(0)
    return out


def _check_invrms_gpu(x, res, w, y, s, ref, msg):
    """GPU only: the fp32 invrms, read through the extension. rtol 1e-5:
    the per-thread chain plus the reduction tree is ~30 additions (2e-6)
    plus rsqrtf; one dropped element at H=4096 moves it by 1.2e-4.
    Largest error observed on an MI355X over all cases here: 1.2e-7
    relative (1.2 % of the bound)."""
    outs = ops._ext().rmsnorm_fwd(
        x.contiguous(), None if res is None else res.contiguous(), w, EPS)
    assert torch.equal(outs[0].reshape(y.shape), y), f"{msg}: y differs between calls"
    if res is not None:
        assert torch.equal(outs[2].reshape(s.shape), s)
    assert outs[1].dtype == torch.float32 and outs[1].numel() == ref["ir"].numel()
    _assert_fp32(outs[1], ref["ir"], rtol=1e-5, msg=f"{msg} invrms")


def _rms_inputs(device, shape, seed):
    g = torch.Generator().manual_seed(seed)
    H = shape[-1]
    x = torch.randn(shape, generator=g).to(BF16).to(device)
    r = torch.randn(shape, generator=g).to(BF16).to(device)
    w = torch.randn(H, generator=g).to(BF16).to(device)
    dy = torch.randn(shape, generator=g).to(BF16).to(device)
    ds = torch.randn(shape, generator=g).to(BF16).to(device)
    return x, r, w, dy, ds


def _run_rmsnorm(device, x, w, dy, msg):
    """ops.rmsnorm forward (+ backward when dy is given) vs float64."""
    xi = x.clone().requires_grad_(True)
    wi = w.clone().requires_grad_(True)
    y = ops.rmsnorm(xi, wi, EPS)
    assert y.dtype == BF16 and y.shape == x.shape
    ref = _ref_rmsnorm64(x, w, dy)
    assert_bf16_ulp(y.reshape(ref["y"].shape), ref["y"], ref["y_extra"], msg=f"{msg} y")
    if device == "cuda":
        _check_invrms_gpu(x, None, w, y.detach(), None, ref, msg)
    if dy is not None:
        y.backward(dy)
        assert_bf16_ulp(xi.grad.reshape(ref["dx"].shape), ref["dx"],
                        ref["dx_extra"], msg=f"{msg} dx")
        assert_bf16_ulp(wi.grad, ref["dw"], ref["dw_extra"], msg=f"{msg} dw")


def _run_add_rmsnorm(device, x, r, w, dy, ds, msg):
    """ops.add_rmsnorm vs float64. dy/ds None = that output is unused
    downstream (autograd then hands the op None for it)."""
    xi = x.clone().requires_grad_(True)
    ri = r.clone().requires_grad_(True)
    wi = w.clone().requires_grad_(True)
    y, s = ops.add_rmsnorm(xi, ri, wi, EPS)
    s_exp = (x.float() + r.float()).to(BF16)
    assert torch.equal(_bits(s), _bits(s_exp)), f"{msg}: s not bit-equal to bf16(x+res)"
    ref = _ref_rmsnorm64(s_exp, w, dy if dy is not None else torch.zeros_like(x), ds)
    assert_bf16_ulp(y.reshape(ref["y"].shape), ref["y"], ref["y_extra"], msg=f"{msg} y")
    if device == "cuda":
        _check_invrms_gpu(x, r, w, y.detach(), s.detach(), ref, msg)
    if dy is None and ds is None:
        return
    outs, grads = [], []
    if dy is not None:
        outs.append(y)
        grads.append(dy)
    if ds is not None:
        outs.append(s)
        grads.append(ds)
    torch.autograd.backward(outs, grads)
    assert torch.equal(_bits(xi.grad), _bits(ri.grad)), f"{msg}: dx != dres"
    assert_bf16_ulp(xi.grad.reshape(ref["dx"].shape), ref["dx"], ref["dx_extra"],
                    msg=f"{msg} dx")
    assert_bf16_ulp(wi.grad, ref["dw"], ref["dw_extra"], msg=f"{msg} dw")
    if dy is None:  # only s used: the gradient is ds itself, dw is zero
        assert torch.equal(_bits(xi.grad), _bits(ds))
        assert not wi.grad.any()


# (N, H). 2056 is the first H with a second loop iteration of a thread;
# 513 and 1029 rows give the 512 backward blocks uneven numbers of rows.
RMS_SHAPES = [(1, 8), (3, 64), (5, 2048), (5, 2056), (513, 64), (1029, 512),
              (520, 4096)]


def _check_rmsnorm(device, N, H):
    x, r, w, dy, ds = _rms_inputs(device, (N, H), seed=N * 10007 + H)
    _run_rmsnorm(device, x, w, dy, f"rmsnorm {N}x{H}")


def _check_add_rmsnorm(device, N, H):
    x, r, w, dy, ds = _rms_inputs(device, (N, H), seed=N * 10009 + H)
    _run_add_rmsnorm(device, x, r, w, dy, ds, f"add_rmsnorm {N}x{H}")


_both("rmsnorm_fwd_bwd", _check_rmsnorm, RMS_SHAPES)
_both("add_rmsnorm_fwd_bwd", _check_add_rmsnorm, RMS_SHAPES)


def _check_rmsnorm_many_rows(device):
    """N > 2048: the forward grid-strides over rows (forward only)."""
    x, r, w, _, _ = _rms_inputs(device, (2051, 64), seed=11)
    _run_rmsnorm(device, x, w, None, "rmsnorm 2051x64")
    _run_add_rmsnorm(device, x, r, w, None, None, "add_rmsnorm 2051x64")


_both("rmsnorm_many_rows", _check_rmsnorm_many_rows)


def _spike_positions(H):
    pos = {0, 7, 8 % H, H - 8, H - 1}
    if H > 2048:
        pos |= {2047, 2048, 2055}
    return sorted(pos)


def _check_rmsnorm_spikes(device, H):
    """Rows that are zero except one large value, at the columns where a
    thread's vector or loop iteration changes: a dropped or duplicated
    element changes such a row completely."""
    pos = _spike_positions(H)
    g = torch.Generator().manual_seed(H)
    x = torch.zeros(len(pos), H)
    for r, p in enumerate(pos):
        x[r, p] = (-1) ** r * (3.0 + r)
    x = x.to(BF16).to(device)
    res = torch.zeros_like(x)
    res[:, 0] += 0.5  # a second non-zero so the fused sum is not trivial
    w = torch.randn(H, generator=g).to(BF16).to(device)
    dy = torch.randn(len(pos), H, generator=g).to(BF16).to(device)
    ds = torch.randn(len(pos), H, generator=g).to(BF16).to(device)
    _run_rmsnorm(device, x, w, dy, f"rmsnorm spikes H={H}")
    _run_add_rmsnorm(device, x, res, w, dy, ds, f"add_rmsnorm spikes H={H}")


_both("rmsnorm_spikes", _check_rmsnorm_spikes, [(8,), (64,), (2048,), (2056,), (4096,)])


def _check_rmsnorm_layouts(device):
    """3-D input and a non-contiguous x (the transpose of a [64, 6] tensor)."""
    x, r, w, dy, ds = _rms_inputs(device, (2, 5, 64), seed=5)
    _run_rmsnorm(device, x, w, dy, "rmsnorm 2x5x64")
    _run_add_rmsnorm(device, x, r, w, dy, ds, "add_rmsnorm 2x5x64")
    x, r, w, dy, ds = _rms_inputs(device, (6, 64), seed=6)
    x, r, dyt = (t.t().contiguous().t() for t in (x, r, dy))  # [64, 6] storage
    assert x.shape == (6, 64) and not x.is_contiguous()
    _run_rmsnorm(device, x, w, dyt, "rmsnorm x.t()")
    _run_add_rmsnorm(device, x, r, w, dy, ds, "add_rmsnorm x.t()")


_both("rmsnorm_layouts", _check_rmsnorm_layouts)


def _check_add_rmsnorm_unused_outputs(device):
    """Only s used downstream (dy is None), and only y used (ds is None)."""
    for N, H in ((5, 2056), (513, 64)):
        x, r, w, dy, ds = _rms_inputs(device, (N, H), seed=N + H)
        _run_add_rmsnorm(device, x, r, w, None, ds, f"add_rmsnorm s-only {N}x{H}")
        _run_add_rmsnorm(device, x, r, w, dy, None, f"add_rmsnorm y-only {N}x{H}")


_both("add_rmsnorm_unused_outputs", _check_add_rmsnorm_unused_outputs)


# ---------------------------------------------------------------------------
# RoPE
# ---------------------------------------------------------------------------
def _ref_rope64(x, cos, sin, sign, oscale):
    """float64 rotate-half RoPE of x [B, S, Hh, D] with the first S table
    rows, and its fp32 term 2**-21*oscale*(|x1*c| + |x2*s|) per output:
    two fp32 products, their sum and the scaling."""
    B, S, Hh, D = x.shape
    x64 = _f64(x)
    x1, x2 = x64[..., : D // 2], x64[..., D // 2:]
    c = _f64(cos[:S]).view(1, S, 1, D // 2)
    s = _f64(sin[:S]).view(1, S, 1, D // 2)
    osc = _f32exact(oscale)
    o1 = (x1 * c - sign * x2 * s) * osc
    o2 = (x2 * c + sign * x1 * s) * osc
    e1 = 2.0 ** -21 * osc * ((x1 * c).abs() + (x2 * s).abs())
    e2 = 2.0 ** -21 * osc * ((x2 * c).abs() + (x1 * s).abs())
    return torch.cat([o1, o2], -1), torch.cat([e1, e2], -1)


# oscale that is no power of two: the softmax scale * log2(e) that the
# model folds into q for the v3 attention path
OSCALE = 128 ** -0.5 * ops.LOG2E

# (B, S, Hh, D, table rows, oscale). D=8 is one quad per head; B=1 with
# several heads keeps the transposed gradient a strided view into the
# backward kernel.
ROPE_CASES = [(2, 5, 3, 64, 16, 1.0), (3, 4, 2, 8, 4, OSCALE),
              (1, 7, 1, 128, 9, OSCALE), (1, 6, 3, 16, 8, 1.0)]


def _check_rope_qkv_views(device, B, S, Hh, D, rows, oscale):
    """q and k taken as views of one fused [B, S, 3*Hh*D] projection, as
    the model does; the consumer transposes the output, so dy arrives
    non-contiguous."""
    g = torch.Generator().manual_seed(B * 1000 + S * 100 + Hh * 10 + D)
    cos, sin = ops.precompute_rope(rows, D, base=10000.0, device=device)
    fused = torch.randn(B, S, 3 * Hh * D, generator=g).to(BF16).to(device)
    wq = torch.randn(B, Hh, S, D, generator=g).to(BF16).to(device)
    wk = torch.randn(B, Hh, S, D, generator=g).to(BF16).to(device)

    fi = fused.clone().requires_grad_(True)
    q, k, v = fi.split([Hh * D] * 3, dim=-1)
    qv, kv = q.view(B, S, Hh, D), k.view(B, S, Hh, D)
    assert not qv.is_contiguous() and not kv.is_contiguous()
    yq = ops.rope(qv, cos, sin, oscale)
    yk = ops.rope(kv, cos, sin, oscale)
    for name, view, y in (("q", qv, yq), ("k", kv, yk)):
        yc = ops.rope(view.detach().contiguous(), cos, sin, oscale)
        assert torch.equal(_bits(y), _bits(yc)), f"rope {name}: view != contiguous"
        ref, extra = _ref_rope64(view, cos, sin, 1.0, oscale)
        assert_bf16_ulp(y, ref, extra, msg=f"rope fwd {name}")

    # the weighted sum makes dy = w.transpose(1, 2) exactly (bf16 product
    # gradients of a sum), a transposed, non-contiguous [B, S, Hh, D]
    loss = (yq.transpose(1, 2) * wq).sum() + (yk.transpose(1, 2) * wk).sum()
    loss.backward()
    dq, dk, dv = fi.grad.split([Hh * D] * 3, dim=-1)
    assert not dv.any()
    for name, dx, wgt in (("q", dq, wq), ("k", dk, wk)):
        ref, extra = _ref_rope64(wgt.transpose(1, 2), cos, sin, -1.0, oscale)
        assert_bf16_ulp(dx.reshape(B, S, Hh, D), ref, extra, msg=f"rope bwd {name}")


_both("rope_qkv_views", _check_rope_qkv_views, ROPE_CASES)


def _check_rope_grid_stride(device):
    """540672 quads > 2048*256 threads: the grid-stride loop (forward)."""
    B, S, Hh, D = 1, 1024, 33, 128
    g = torch.Generator().manual_seed(12)
    cos, sin = ops.precompute_rope(S + 6, D, base=10000.0, device=device)
    x = torch.randn(B, S, Hh, D, generator=g).to(BF16).to(device)
    y = ops.rope(x, cos, sin)
    ref, extra = _ref_rope64(x, cos, sin, 1.0, 1.0)
    assert_bf16_ulp(y, ref, extra, msg="rope grid-stride")


_both("rope_grid_stride", _check_rope_grid_stride)


# ---------------------------------------------------------------------------
# SwiGLU
# ---------------------------------------------------------------------------
_GATES = [0.0, 1e-3, 1.0, 10.0, 20.0, 50.0, 88.0, 89.0, 100.0, 1e4]
GATES = _GATES + [-g for g in _GATES]  # exp(-g) overflows fp32 past |g|=88


def _swiglu_inputs(device, N, I):
    g = torch.Generator().manual_seed(N * 31 + I)
    vals = torch.tensor(GATES)
    idx = (torch.arange(I).view(1, I) + torch.arange(N).view(N, 1)) % len(GATES)
    gate = vals[idx]
    # every second row random, so ordinary values are covered too
    gate[1::2] = torch.randn(gate[1::2].shape, generator=g) * 3
    up = torch.randn(N, I, generator=g)
    gu = torch.cat([gate, up], -1).to(BF16).to(device)
    dout = torch.randn(N, I, generator=g).to(BF16).to(device)
    return gu, dout


def _ref_swiglu64(gu, dout):
    """float64 SwiGLU forward and backward with their fp32 terms.
    sigmoid = 1/(1+exp(-g)) is computed as exp2(-g*log2e): the fp32
    product carries |g|*2**-24 into the exponent, so sigmoid has a relative
    error of about (|g| + 8)*2**-23 with the exp2, add and reciprocal.
    The factor 1 + g*(1 - sig) of dgate adds the error of 1 - sig, one ulp
    of 1, times |g|; past g = 18 the fp32 sigmoid is exactly 1 and the
    factor exactly 1, so |g| is capped there."""
    I = gu.shape[-1] // 2
    g, u = _f64(gu[..., :I]), _f64(gu[..., I:])
    do = _f64(dout)
    sig = torch.sigmoid(g)
    rel = 2.0 ** -23 * (g.abs() + 8)
    out = g * sig * u
    dg = do * u * sig * (1 + g * (1 - sig))
    du = do * g * sig
    dg_extra = rel * dg.abs() + 2.0 ** -21 * (1 + g.abs().clamp(max=18)) * (do * u * sig).abs()
    return (out, rel * out.abs(), torch.cat([dg, du], -1),
            torch.cat([dg_extra, rel * du.abs()], -1))


def _check_swiglu(device, N, I):
    gu, dout = _swiglu_inputs(device, N, I)
    gi = gu.clone().requires_grad_(True)
    y = ops.swiglu(gi)
    y.backward(dout)
    out, out_extra, dgu, dgu_extra = _ref_swiglu64(gu, dout)
    assert_bf16_ulp(y, out, out_extra, msg=f"swiglu fwd {N}x{I}")
    assert_bf16_ulp(gi.grad, dgu, dgu_extra, msg=f"swiglu bwd {N}x{I}")


# 2050*2048/8 = 524800 vectors > 2048*256 threads: the grid-stride loop
_both("swiglu", _check_swiglu, [(1, 8), (3, 24), (65, 136), (2050, 2048)])


# ---------------------------------------------------------------------------
# Fused cross-entropy
# ---------------------------------------------------------------------------
IGNORE = -100


def _ref_ce64(logits, targets, scale=1.0):
    """float64 per-row loss, mean loss over valid rows, and the gradient of
    `scale` * sum of row losses (ignored rows: loss 0, gradient 0)."""
    V = logits.shape[-1]
    x = _f64(logits).reshape(-1, V)
    t = targets.reshape(-1)
    valid = t != IGNORE
    tc = t.clamp(min=0)
    lse = torch.logsumexp(x, -1)
    rows = torch.where(valid, lse - x.gather(1, tc.view(-1, 1)).squeeze(1),
                       torch.zeros_like(lse))
    p = torch.softmax(x, -1)
    p.scatter_add_(1, tc.view(-1, 1), -torch.ones_like(lse).view(-1, 1))
    grad = torch.where(valid.view(-1, 1), p, torch.zeros_like(p)) * scale
    n_valid = max(int(valid.sum()), 1)
    return rows, rows.sum() / n_valid, grad, n_valid


def _loss_cap(V):
    """The fp32 loss bound never reaches 1/(4V), a quarter of what one
    dropped average logit does to a row's loss."""
    return 0.9 / (4 * V)


def _run_ce(device, logits, targets, msg, gout=1.0):
    """ops.fused_cross_entropy (mean loss, gradient of gout*loss) and, on
    GPU, the per-row loss and scaled gradient through the extension.

    Loss bound: atol 2e-5*max(1, |ref|), held below 1/(4V). Largest
    per-row error observed on an MI355X over all cases here: 1.5e-6
    (2.7 % of its bound); mean loss 0.7 % of its bound.
    Gradient: ulp rule with extra_abs=1e-5. The op stores softmax - onehot
    rounded to bf16 and backward multiplies that by gout/n_valid and
    rounds again. So the rule is applied to the stored gradient (gout =
    n_valid makes the factor exactly 1), and the gradient of gout*loss
    must be bit-equal to that gradient times fp32(gout/n_valid), rounded
    once. Where the factor is a power of two the second rounding is exact
    and the rule is applied to the scaled gradient as well."""
    V = logits.shape[-1]
    rows, mean, grad, n_valid = _ref_ce64(logits, targets)
    grad = grad.reshape(logits.shape)
    lu = logits.clone().requires_grad_(True)
    (ops.fused_cross_entropy(lu, targets, IGNORE) * float(n_valid)).backward()
    assert_bf16_ulp(lu.grad, grad, extra_abs=1e-5, msg=f"{msg} stored grad")
    li = logits.clone().requires_grad_(True)
    loss = ops.fused_cross_entropy(li, targets, IGNORE)
    (loss * gout).backward()
    _assert_fp32(loss, mean, atol=2e-5, cap=_loss_cap(V), msg=f"{msg} mean loss")
    factor = (torch.tensor(gout, dtype=torch.float32, device=device)
              / torch.tensor(n_valid, device=device)).item()
    want = (lu.grad.float() * factor).to(BF16)
    assert torch.equal(_bits(li.grad), _bits(want)), f"{msg}: grad != stored*gout/n"
    if math.frexp(factor)[0] == 0.5:
        assert_bf16_ulp(li.grad, grad * factor, extra_abs=1e-5, msg=f"{msg} grad")
    masked = logits == float("-inf")
    assert not li.grad[masked].any(), f"{msg}: gradient on masked columns"
    ignored = (targets == IGNORE)
    assert not li.grad[ignored].any(), f"{msg}: gradient on ignored rows"
    if device == "cuda":
        scale = 0.37
        buf = logits.clone().reshape(-1, V)
        got = ops._ext().cross_entropy_fwd_(buf, targets.reshape(-1).contiguous(),
                                            scale, IGNORE)
        _assert_fp32(got, rows, atol=2e-5, cap=_loss_cap(V), msg=f"{msg} row loss")
        assert_bf16_ulp(buf, grad.reshape(-1, V) * _f32exact(scale), extra_abs=1e-5,
                        msg=f"{msg} ext grad")
        assert not buf[masked.reshape(-1, V)].any()
        assert not buf[ignored.reshape(-1)].any()
        assert not got[ignored.reshape(-1)].any()


def _ce_spike_rows(V):
    """Zero rows with one spike, the row maximum, at the columns where a
    thread's vector or loop iteration changes; the target once on the
    spike, once at column 0 and once at V-1."""
    rows, tgts = [], []
    for p in _spike_positions(V):
        for t in (p, 0, V - 1):
            row = torch.zeros(V)
            row[p] = 8.0
            rows.append(row)
            tgts.append(t)
    return torch.stack(rows), torch.tensor(tgts)


def _check_ce(device, V):
    g = torch.Generator().manual_seed(V)
    spikes, t_spk = _ce_spike_rows(V)
    # at least 16 random rows; the row count is filled up to a power of two
    # so that the mean's 1/n_valid is exact in bf16 (see _run_ce)
    n_rnd = 16
    while (n_rnd + len(spikes)) & (n_rnd + len(spikes) - 1):
        n_rnd += 1
    rnd = torch.randn(n_rnd, V, generator=g) * 4
    rnd[14] = torch.linspace(-30, 30, V)  # every element rescales the sum
    rnd[15] = torch.linspace(30, -30, V)  # none does
    t_rnd = torch.randint(0, V, (n_rnd,), generator=g)
    logits = torch.cat([rnd, spikes]).to(BF16).to(device)
    targets = torch.cat([t_rnd, t_spk]).to(device)
    _run_ce(device, logits, targets, f"ce V={V}")


_both("ce_vocab", _check_ce, [(8,), (64,), (2048,), (2056,), (4104,)])


def _check_ce_scaled_and_3d(device):
    """loss*3 backward at the wrapper level, and 3-D logits."""
    g = torch.Generator().manual_seed(3)
    logits = (torch.randn(2, 5, 64, generator=g) * 4).to(BF16).to(device)
    targets = torch.randint(0, 64, (2, 5), generator=g).to(device)
    _run_ce(device, logits, targets, "ce 2x5x64 loss*3", gout=3.0)
    logits = (torch.randn(16, 2056, generator=g) * 4).to(BF16).to(device)
    targets = torch.randint(0, 2056, (16,), generator=g).to(device)
    _run_ce(device, logits, targets, "ce 16x2056 loss*3", gout=3.0)


_both("ce_scaled_and_3d", _check_ce_scaled_and_3d)


def _check_ce_ignore(device):
    """N > 2048 rows: the row grid-stride, with ignored rows (the
    `continue` path) before and after a valid row of the same block."""
    N, V = 2051, 64
    g = torch.Generator().manual_seed(4)
    logits = (torch.randn(N, V, generator=g) * 4).to(BF16).to(device)
    targets = torch.randint(0, V, (N,), generator=g)
    targets[torch.rand(N, generator=g) < 0.2] = IGNORE
    targets[0], targets[2049] = IGNORE, IGNORE
    targets[2048], targets[1] = 5, 63
    targets = targets.to(device)
    _run_ce(device, logits, targets, "ce ignore 2051x64")
    # all rows ignored: loss 0, gradient 0
    allig = torch.full((N,), IGNORE, device=device)
    li = logits.clone().requires_grad_(True)
    loss = ops.fused_cross_entropy(li, allig, IGNORE)
    loss.backward()
    assert loss.item() == 0.0
    assert not li.grad.any()


_both("ce_ignore", _check_ce_ignore)


def _check_ce_masked(device, V):
    """-inf logits (masked vocabulary): finite loss equal to float64 and
    exactly zero gradient on the masked columns. A thread owns columns
    8*t..8*t+7 of every 2048."""
    NEG = float("-inf")
    g = torch.Generator().manual_seed(V + 1)
    x = torch.randn(6, V, generator=g) * 4
    x[0, 0:8] = NEG                      # seen before any finite value
    x[1, 24:32] = NEG                    # all of thread 3's share ...
    x[1, 0:8] = NEG                      # ... and of thread 0's
    if V > 2048:
        x[1, 2048 + 24:2048 + 32] = NEG
        x[1, 2048:2056] = NEG
    x[2, 0::2] = NEG                     # interleaved, -inf first
    x[3, 1::2] = NEG                     # interleaved, finite first
    x[4, 8:] = NEG                       # only thread 0's first vector left
    x[5, :V - 1] = NEG                   # a single finite logit, the last
    targets = torch.tensor([8, 40, 1, V - 2, 3, V - 1])
    assert not x[torch.arange(6), targets].isinf().any()  # target never masked
    _run_ce(device, x.to(BF16).to(device), targets.to(device), f"ce masked V={V}")


_both("ce_masked", _check_ce_masked, [(64,), (2056,)])


# ---------------------------------------------------------------------------
# AdamW
# ---------------------------------------------------------------------------
# exactly representable in fp32, so the reference needs no guess about
# how the kernel rounds 1.f - beta
ADAM = dict(lr=2.0 ** -7, beta1=0.875, beta2=0.9375, eps=2.0 ** -27, wd=0.125,
            grad_scale=0.5)


def _adam_step_check(p, g, m, v, step, msg):
    """One ops.adamw_ step on (views of) p, g, m, v against float64 seeded
    from the kernel's own state before the step, so errors do not compound.
    m: rtol 1e-6 plus 2**-23*(|b1*m| + |(1-b1)*g|) for the fp32 sum of two
    terms of opposite sign; v (all terms positive): rtol 1e-6; p: ulp rule
    with the fp32 term 2**-21*(|p| + lr*(|update| + wd*|p|))."""
    h = ADAM
    p0, m0, v0 = _f64(p), _f64(m), _f64(v)
    gs = _f64(g) * h["grad_scale"]
    ops.adamw_(p, g, m, v, h["lr"], h["beta1"], h["beta2"], h["eps"], h["wd"],
               step, h["grad_scale"])
    m1 = h["beta1"] * m0 + (1 - h["beta1"]) * gs
    v1 = h["beta2"] * v0 + (1 - h["beta2"]) * gs * gs
    upd = (m1 / (1 - h["beta1"] ** step)) / ((v1 / (1 - h["beta2"] ** step)).sqrt() + h["eps"])
    p1 = p0 - h["lr"] * (upd + h["wd"] * p0)
    m_err = (_f64(m) - m1).abs()
    m_bound = 1e-6 * m1.abs() + 2.0 ** -23 * ((h["beta1"] * m0).abs()
                                              + ((1 - h["beta1"]) * gs).abs())
    assert bool((m_err <= m_bound).all()), f"{msg}: m off by {(m_err - m_bound).max().item():.3e}"
    v_err = (_f64(v) - v1).abs()
    assert bool((v_err <= 1e-6 * v1.abs()).all()), \
        f"{msg}: v off, worst relative {(v_err / v1.abs().clamp(min=1e-300)).max().item():.3e}"
    extra = 2.0 ** -21 * (p0.abs() + h["lr"] * (upd.abs() + h["wd"] * p0.abs()))
    assert_bf16_ulp(p, p1, extra, msg=f"{msg} p")


def _check_adamw(device, n):
    """n < 8: tail kernel alone; n % 8 == 0: no tail; 4194317 > 2048*256*8:
    grid-stride plus tail."""
    gen = torch.Generator().manual_seed(n)
    p = torch.randn(n, generator=gen).to(BF16).to(device)
    m = torch.zeros(n, dtype=torch.float32, device=device)
    v = torch.zeros(n, dtype=torch.float32, device=device)
    for step in (1, 2, 3):
        g = torch.randn(n, generator=gen).to(BF16).to(device)
        g0 = g.clone()
        _adam_step_check(p, g, m, v, step, f"adamw n={n} step {step}")
        assert torch.equal(_bits(g), _bits(g0)), "adamw changed g"


_both("adamw", _check_adamw, [(1,), (7,), (8,), (9,), (1003,), (4194317,)])


def _check_adamw_slice(device, n):
    """The ZeRO path steps a slice of the flat bucket. Offset 8 keeps the
    16-byte alignment that the bucket padding (to 8, and shards to world*8
    elements) gives every slice. Nothing outside [8, 8+n) may change."""
    gen = torch.Generator().manual_seed(100 + n)
    P = torch.full((n + 16,), -7.0, dtype=BF16, device=device)
    G = torch.full((n + 16,), 3.0, dtype=BF16, device=device)
    M = torch.full((n + 16,), 5.0, dtype=torch.float32, device=device)
    V = torch.full((n + 16,), 9.0, dtype=torch.float32, device=device)
    sl = slice(8, 8 + n)
    P[sl] = torch.randn(n, generator=gen).to(BF16).to(device)
    G[sl] = torch.randn(n, generator=gen).to(BF16).to(device)
    M[sl] = torch.randn(n, generator=gen).to(device) * 0.1
    V[sl] = torch.rand(n, generator=gen).to(device) * 0.1
    before = [t.clone() for t in (P, G, M, V)]
    assert P[sl].data_ptr() % 16 == 0
    _adam_step_check(P[sl], G[sl], M[sl], V[sl], 2, f"adamw slice n={n}")
    assert torch.equal(_bits(G), _bits(before[1])), "adamw changed g"
    for name, t, b in zip("pmv", (P, M, V), (before[0], before[2], before[3])):
        assert torch.equal(_bits(t[:8]), _bits(b[:8])), f"adamw wrote before {name}"
        assert torch.equal(_bits(t[8 + n:]), _bits(b[8 + n:])), f"adamw wrote past {name}"
        assert not torch.equal(_bits(t[sl]), _bits(b[sl]))


_both("adamw_slice_guard", _check_adamw_slice, [(1,), (7,), (8,), (9,), (1003,)])


# ---------------------------------------------------------------------------
# pack / unpack
# ---------------------------------------------------------------------------
def _pack_values(n, dtype, gen):
    if dtype == torch.uint8:
        return torch.randint(0, 255, (n,), generator=gen, dtype=torch.uint8)
    return torch.randn(n, generator=gen).to(dtype)


def _sentinel(n, dtype, device):
    return torch.full((n,), 165 if dtype == torch.uint8 else -123.0,
                      dtype=dtype, device=device)


def _check_pack(device, dtype, sizes):
    dtype = getattr(torch, dtype)
    es = dtype.itemsize
    gen = torch.Generator().manual_seed(sum(sizes) + es)
    ts = [_pack_values(n, dtype, gen).to(device) for n in sizes]
    offs, total = ops.aligned_offsets(sizes, es)
    # pack into a sentinel-filled buffer: padding keeps the sentinel
    flat, got_offs = ops.pack_tensors(ts, flat=_sentinel(total, dtype, device))
    assert got_offs == offs and flat.numel() == total
    want = _sentinel(total, dtype, device)
    for t, o in zip(ts, offs):
        want[o:o + t.numel()] = t
    assert torch.equal(_bits(flat), _bits(want)), "pack"
    # a fresh buffer is zero in the padding
    flat0, _ = ops.pack_tensors(ts)
    want0 = torch.zeros(total, dtype=dtype, device=device)
    for t, o in zip(ts, offs):
        want0[o:o + t.numel()] = t
    assert torch.equal(_bits(flat0), _bits(want0)), "pack into fresh buffer"
    # unpack into 16-byte-aligned slices of a sentinel buffer: the gaps
    # between the slices keep the sentinel
    step = ops.PACK_ALIGN // es
    buf = _sentinel(total + 2 * step, dtype, device)
    outs = [buf[step + o:step + o + n] for o, n in zip(offs, sizes)]
    assert all(t.data_ptr() % 16 == 0 for t in outs)
    ops.unpack_tensors(flat, outs, offsets=offs)
    wantb = _sentinel(total + 2 * step, dtype, device)
    for t, o in zip(ts, offs):
        wantb[step + o:step + o + t.numel()] = t
    assert torch.equal(_bits(buf), _bits(wantb)), "unpack"


_MIB4 = 4 * 1024 * 1024
PACK_CASES = [
    ("bfloat16", (3, 0, 1000, 1, 8, 13)),        # an empty tensor between others
    ("bfloat16", (1001,)),                       # a single segment
    ("float32", (1, 2, 3, 5, 0, 4, 1023)),       # byte tails 4, 8, 12
    ("uint8", tuple(range(1, 16)) + (16, 17, 31, 0, 33)),  # byte tails 1..15
    ("uint8", (5, _MIB4 + 21, 3)),               # above 4 MiB: grid-stride in x
    ("float32", (_MIB4 // 4 + 7,)),
]
_both("pack_unpack", _check_pack, PACK_CASES)


class _NoPackKernel:
    """Stands in for the extension; a pack kernel launch is an error."""

    def __init__(self, ext):
        self._ext = ext

    def __getattr__(self, name):
        if name == "pack_segments":
            raise AssertionError("pack kernel launched for a misaligned tensor")
        return getattr(self._ext, name)


def _check_pack_misaligned(device, monkeypatch):
    """A t[1:] view is contiguous and not 16-byte aligned: such calls take
    the per-tensor copy, never the 16-byte-vector kernel."""
    gen = torch.Generator().manual_seed(8)
    base = torch.randn(1000, generator=gen).to(BF16).to(device)
    a = torch.randn(24, generator=gen).to(BF16).to(device)
    mis = base[1:]
    assert mis.is_contiguous()
    if device == "cuda":
        assert base.data_ptr() % 16 == 0 and mis.data_ptr() % 16 == 2
        proxy = _NoPackKernel(ops._ext())
        monkeypatch.setattr(ops, "_ext", lambda: proxy)
    flat, offs = ops.pack_tensors([a, mis, a])
    want = torch.zeros(flat.numel(), dtype=BF16, device=device)
    for t, o in zip([a, mis, a], offs):
        want[o:o + t.numel()] = t
    assert torch.equal(_bits(flat), _bits(want))
    dst = torch.full((1000,), -123.0, dtype=BF16, device=device)
    outs = [torch.zeros_like(a), dst[1:], torch.zeros_like(a)]
    ops.unpack_tensors(flat, outs, offsets=offs)
    assert torch.equal(_bits(dst[1:]), _bits(mis)) and dst[0].item() == -123.0
    assert torch.equal(_bits(outs[0]), _bits(a)) and torch.equal(_bits(outs[2]), _bits(a))


def test_pack_misaligned_cpu(monkeypatch):
    _check_pack_misaligned("cpu", monkeypatch)


@pytest.mark.gpu
def test_pack_misaligned_gpu(monkeypatch):
    _check_pack_misaligned("cuda", monkeypatch)


# ---------------------------------------------------------------------------
# Attention (GPU only, D = 128)
# ---------------------------------------------------------------------------
def _ref_attn64(q, k, v, scale):
    """float64 causal GQA attention on [B, H, S, D]; returns (o, lse)."""
    g = q.shape[1] // k.shape[1]
    S = q.shape[2]
    k = k.repeat_interleave(g, 1)
    v = v.repeat_interleave(g, 1)
    s = (q @ k.transpose(-1, -2)) * scale
    s = s + torch.full((S, S), float("-inf"), dtype=F64, device=q.device).triu(1)
    return torch.softmax(s, -1) @ v, torch.logsumexp(s, -1)


def _close(a, b, atol=2e-2, rtol=2e-2, msg=""):
    torch.testing.assert_close(_f64(a), _f64(b), rtol=rtol, atol=atol, msg=msg)


def _leaf64(t):
    return _f64(t).requires_grad_(True)


@pytest.mark.gpu
@pytest.mark.parametrize("B,Hq,Hkv,S", [(2, 4, 2, 256), (1, 4, 1, 384)])
def test_attn_fwd_wmma_gqa_gpu(B, Hq, Hkv, S):
    """rocWMMA kernel: GQA head mapping (K/V differ per kv head), B > 1, an
    odd number of 128-row tiles. o under 2e-2; LSE under the fp32 rule,
    atol 2e-5*max(1, |ref|). Largest LSE error observed on an MI355X:
    7.7e-7 (0.9 % of its bound)."""
    torch.manual_seed(B * 100 + S)
    scale = 128 ** -0.5
    q = torch.randn(B, Hq, S, 128, dtype=BF16, device="cuda")
    k = torch.randn(B, Hkv, S, 128, dtype=BF16, device="cuda")
    v = torch.randn(B, Hkv, S, 128, dtype=BF16, device="cuda")
    o, lse = ops._ext().attn_fwd(q, k, v, scale)
    o_ref, lse_ref = _ref_attn64(_f64(q), _f64(k), _f64(v), _f32exact(scale))
    _close(o, o_ref, msg="wmma o")
    _assert_fp32(lse, lse_ref, atol=2e-5, cap=_loss_cap(S), msg=f"wmma S={S} lse")


def _attn_fwd_bwd_vs_fp64(impl, B, Hq, Hkv, S, transposed, scale, close_grad):
    """ops.flash_attention forward + backward against float64 SDPA, with
    q, k, v optionally built [B, S, H, D] and passed as transposed views."""
    D = 128

    def make(H):
        if transposed:
            return torch.randn(B, S, H, D, dtype=BF16, device="cuda")
        return torch.randn(B, H, S, D, dtype=BF16, device="cuda")
    q0, k0, v0 = make(Hq), make(Hkv), make(Hkv)
    if impl == "v3":  # contract: q pre-scaled by scale*log2e, rounded once
        q0 = (q0.float() * (D ** -0.5 * ops.LOG2E)).to(BF16)
    leaves = [t.clone().requires_grad_(True) for t in (q0, k0, v0)]
    ins = [t.transpose(1, 2) if transposed else t for t in leaves]
    if transposed:
        assert not ins[0].is_contiguous()
    out = ops.flash_attention(*ins, impl=impl)
    gout = torch.randn(B, Hq, S, D, dtype=BF16, device="cuda")
    out.backward(gout)

    refs = [_leaf64(t) for t in (q0, k0, v0)]
    rin = [t.transpose(1, 2) if transposed else t for t in refs]
    o_ref, _ = _ref_attn64(*rin, scale)
    o_ref.backward(_f64(gout))
    _close(out, o_ref, msg=f"{impl} o")
    for name, a, b in zip("qkv", leaves, refs):
        close_grad(a.grad, b.grad, f"{impl} d{name}")
    if transposed:  # the same call on contiguous copies gives the same bits
        with torch.no_grad():
            oc = ops.flash_attention(*[t.detach().contiguous() for t in ins], impl=impl)
        assert torch.equal(_bits(out), _bits(oc)), f"{impl}: view != contiguous"


@pytest.mark.gpu
def test_flash_attention_wmma_gqa_fwd_bwd_gpu():
    torch.manual_seed(21)
    _attn_fwd_bwd_vs_fp64("wmma", 2, 4, 2, 256, False, _f32exact(128 ** -0.5),
                          lambda a, b, m: _close(a, b, msg=m))


@pytest.mark.gpu
def test_flash_attention_ck_transposed_views_gpu():
    """impl="ck" with [B, S, H, D] tensors passed as transposed views, as
    the model feeds it; tolerances of TestFlashAttention.test_fwd_bwd_gqa."""
    torch.manual_seed(22)
    _attn_fwd_bwd_vs_fp64("ck", 2, 4, 2, 384, True, _f32exact(128 ** -0.5),
                          lambda a, b, m: _close(a, b, msg=m))


@pytest.mark.gpu
def test_flash_attention_v3_transposed_views_gpu():
    """impl="v3" likewise; gradient tolerance of
    TestFlashAttention.test_v3_prescaled_fwd_bwd (magnitude-aware atol)."""
    torch.manual_seed(23)

    def close_rel(a, b, msg):
        _close(a, b, atol=max(2e-2, 6e-3 * b.abs().max().item()), msg=msg)
    _attn_fwd_bwd_vs_fp64("v3", 2, 4, 2, 256, True, ops._LN2, close_rel)


# ---------------------------------------------------------------------------
# Host-side argument checks: these raise before any launch
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_host_argument_checks_gpu():
    def t(*shape):
        return torch.zeros(shape, dtype=BF16, device="cuda")
    with pytest.raises(RuntimeError):
        ops.rmsnorm(t(4, 12), t(12))
    with pytest.raises(RuntimeError):
        ops.fused_cross_entropy(t(4, 12), torch.zeros(4, dtype=torch.long, device="cuda"))
    with pytest.raises(RuntimeError):
        ops.swiglu(t(4, 24))
    cos, sin = ops.precompute_rope(4, 12, device="cuda")
    with pytest.raises(RuntimeError):
        ops.rope(t(1, 4, 2, 12), cos, sin)


@pytest.mark.gpu
def test_rmsnorm_bwd_argument_checks_gpu():
    ext = ops._ext()
    ir = torch.ones(4, dtype=torch.float32, device="cuda")

    def t(*shape):
        return torch.zeros(shape, dtype=BF16, device="cuda")
    ext.rmsnorm_bwd(t(4, 16), None, t(4, 16), t(16), ir)  # well-formed
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ext.rmsnorm_bwd(t(4, 12), None, t(4, 12), t(12), ir)
    with pytest.raises(RuntimeError, match="dy shape"):
        ext.rmsnorm_bwd(t(3, 16), None, t(4, 16), t(16), ir)
    with pytest.raises(RuntimeError, match="ds shape"):
        ext.rmsnorm_bwd(t(4, 16), t(4, 8), t(4, 16), t(16), ir)
    with pytest.raises(RuntimeError, match="invrms"):
        ext.rmsnorm_bwd(t(4, 16), None, t(4, 16), t(16), ir[:3])
    with pytest.raises(RuntimeError, match="invrms"):
        ext.rmsnorm_bwd(t(4, 16), None, t(4, 16), t(16), ir.double())
    # 65536 fp32 = 256 KiB of LDS, more than a CU has
    with pytest.raises(RuntimeError, match="LDS"):
        ext.rmsnorm_bwd(t(1, 65536), None, t(1, 65536), t(65536), ir[:1])


@pytest.mark.gpu
def test_swiglu_bwd_argument_checks_gpu():
    ext = ops._ext()

    def t(*shape):
        return torch.zeros(shape, dtype=BF16, device="cuda")
    ext.swiglu_bwd(t(4, 16), t(4, 32))  # well-formed
    with pytest.raises(RuntimeError, match="dout shape"):
        ext.swiglu_bwd(t(4, 8), t(4, 32))
    with pytest.raises(RuntimeError, match="dout shape"):
        ext.swiglu_bwd(t(3, 16), t(4, 32))
    with pytest.raises(RuntimeError, match="multiple of 16"):
        ext.swiglu_bwd(t(4, 12), t(4, 24))
