"""Dense causal attention: attn_fwd (rocWMMA), attn_fwd_ck, attn_fwd_ck_tr,
attn_fwd_v3, attn_bwd_ck (all four KT_CKBWD_PIPE instantiations) and
ops.flash_attention with its default (aten) backward.

Same scheme as tests/test_paged_attention.py: results are compared with a
float64 reference built from the same bf16 inputs under the one-bf16-ulp
rule (assert_bf16_ulp, copied from there) with a derived per-element term,
at the smallest shapes at which each path exists and over value families
built to make one kind of error gross (see FAMILIES). The rule is proven on
any machine before it is used: the *_cpu tests run a tile-wise emulation of
a flash kernel written here (fp32 scores, online softmax over 64-key tiles,
P and dS rounded to bf16, fp32 accumulation, bf16 outputs), assert that it
passes, and that the same emulation with a one-key leak or a dropped
diagonal at a tile edge fails.

Lines starting with "[edges]" report measured err / bound; run with -s.
"""
import functools
import math

import pytest
import torch

from kubetorch_amd import ops

BF16 = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
D = 128

# (B, Hq, Hkv, S)
S128 = (1, 1, 1, 128)    # one 128-row tile, diagonal only
MHA = (1, 2, 2, 256)     # g = 1
G3 = (2, 6, 2, 384)      # g = 3, odd 128-tile count, B > 1
G8 = (1, 8, 1, 512)      # g = 8
V3X3 = (2, 4, 2, 768)    # three of v3's 256-row tiles

KERNEL_SHAPES = {
    "wmma": [MHA, G3, G8],
    "ck": [S128, MHA, G3, G8],
    "ck_tr": [S128, MHA, G3, G8, V3X3],
    "v3": [MHA, G8, V3X3],
}
BINDING = {"wmma": "attn_fwd", "ck": "attn_fwd_ck", "ck_tr": "attn_fwd_ck_tr",
           "v3": "attn_fwd_v3"}
GRAD_FAMILIES = ["randn", "tempt_next", "rising_max", "offset_minus"]
PIPES = [0, 1, 2, 3]
EDGE_T = [1, 64, 65, 128, 129]  # plus S - 1


def _f64(t):
    return t.detach().to(F64)


def _f32exact(v):
    """A Python float rounded to fp32, as the launchers receive it."""
    return float(torch.tensor(v, dtype=F32))


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


def assert_bf16_ulp(actual, ref64, extra_abs=0, floor=1e-30, msg=""):
    """bf16 result against a float64 reference.

    Hard bound, every element: |a - ref| <= 2**-7*|ref| + extra_abs + floor.
    That is one bf16 ulp: half an ulp of output rounding plus a flip at a
    rounding boundary caused by fp32 ordering.
    Cap: at most 0.1 % of the elements exceed half an ulp,
    2**-8*|ref|*(1 + 2**-10) + extra_abs + floor.
    NaN and inf positions must match the reference exactly. `floor` excuses
    flush-to-zero of results below 1e-30 and nothing else; `extra_abs` is
    the op's accumulation term (a tensor or a number), derived where it is
    used.
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


def _check_ulp(name, actual, ref, extra):
    """Print err / bound and its worst element, then apply the rule."""
    a, r = _f64(actual).cpu(), ref
    ratio = (a - r).abs() / (2.0 ** -7 * r.abs() + extra + 1e-30)
    ratio = torch.where(ratio.isnan(), torch.full_like(ratio, math.inf), ratio)
    i = int(ratio.argmax())
    at = tuple(int(x) for x in torch.unravel_index(torch.tensor(i), r.shape))
    _note(f"{name}_err_over_bound", ratio.reshape(-1)[i].item())
    print(f"[edges] {name}_worst_at {at}")
    assert_bf16_ulp(actual, ref, extra, msg=name)


def _lse_bound(ref, S):
    """The project's fp32 rule (test_attn_fwd_wmma_gqa_gpu): atol
    2e-5*max(1, |ref|), the whole bound held below 0.9/(4*S)."""
    return (2e-5 * ref.abs().clamp(min=1.0)).clamp(max=0.9 / (4 * S))


def _check_lse(name, lse, ref, S):
    a = _f64(lse).cpu()
    assert a.shape == ref.shape, name
    assert bool(a.isfinite().all()), f"{name}: non-finite lse"
    ratio = (a - ref).abs() / _lse_bound(ref, S)
    i = int(ratio.argmax())
    at = tuple(int(x) for x in torch.unravel_index(torch.tensor(i), ref.shape))
    _note(f"{name}_err_over_bound", ratio.reshape(-1)[i].item())
    print(f"[edges] {name}_worst_at {at}")
    assert ratio.reshape(-1)[i].item() <= 1.0, (
        f"{name}: worst got {a.reshape(-1)[i].item()!r}, reference "
        f"{ref.reshape(-1)[i].item()!r} at {at}")


# ---------------------------------------------------------------------------
# Value families: (B, Hq, Hkv, S, gen) -> q, k in fp32; _case rounds them to
# bf16 and draws v, which is randn everywhere, different per kv head and
# batch, so a wrong head or batch mapping is a gross error.
# ---------------------------------------------------------------------------
def _randn(gen, *shape):
    return torch.randn(*shape, generator=gen)


def _signs(gen, *shape):
    """Random +-1 (exact in bf16)."""
    return torch.randint(0, 2, shape, generator=gen).float() * 2 - 1


def _head_factor(Hq, Hkv, span):
    """1 + span * (index in group) / g per query head: the heads of one
    group get different q where the family's q is not built from k."""
    g = Hq // Hkv
    return (1 + span * (torch.arange(Hq) % g).float() / g).view(1, Hq, 1, 1)


def _fam_randn(B, Hq, Hkv, S, gen):
    return _randn(gen, B, Hq, S, D), _randn(gen, B, Hkv, S, D)


def _fam_needle_diag(B, Hq, Hkv, S, gen):
    """q[i] = 4 k[i]: row i puts weight > 1 - 1e-9 on its diagonal key, so
    a mask that drops the diagonal anywhere is a gross error."""
    k = _signs(gen, B, Hkv, S, D)
    return 4 * k.repeat_interleave(Hq // Hkv, 1), k


def _fam_needle_key0(B, Hq, Hkv, S, gen):
    """q[i] = 4 k[0]: the maximum is found in the first tile, every later
    tile is negligible and the first accumulator is rescaled by 1."""
    k = _signs(gen, B, Hkv, S, D)
    q = 4 * k[:, :, :1].expand(B, Hkv, S, D)
    return q.repeat_interleave(Hq // Hkv, 1), k


def _fam_tempt_next(B, Hq, Hkv, S, gen):
    """q[i] = 4 k[i+1] (last row: k[0]): the one key that would dominate
    the row is the first masked one; a one-key leak moves o[i] to v[i+1]."""
    k = _signs(gen, B, Hkv, S, D)
    return 4 * k.roll(-1, 2).repeat_interleave(Hq // Hkv, 1), k


def _fam_rising_max(B, Hq, Hkv, S, gen):
    """k[j] = 2 (j/S) u + 0.25 randn, q = 2 u: the running max rises in
    every tile, so the rescale path runs at every step."""
    u = _signs(gen, B, Hkv, 1, D)
    ramp = (torch.arange(S).float() / S).view(1, 1, S, 1)
    k = 2 * ramp * u + 0.25 * _randn(gen, B, Hkv, S, D)
    q = 2 * u.repeat_interleave(Hq // Hkv, 1) * _head_factor(Hq, Hkv, 0.5)
    return q.expand(B, Hq, S, D), k


def _fam_offset(sign, B, Hq, Hkv, S, gen):
    """k = u + 0.125 randn, q = +-16 u: all scaled scores sit near +-180;
    exponentiating before subtracting the max overflows or gives 0."""
    u = _signs(gen, B, Hkv, 1, D)
    k = u + 0.125 * _randn(gen, B, Hkv, S, D)
    q = sign * 16 * u.repeat_interleave(Hq // Hkv, 1) \
        * _head_factor(Hq, Hkv, 0.25)
    return q.expand(B, Hq, S, D), k


def _fam_q_zero(B, Hq, Hkv, S, gen):
    """q = 0: uniform attention, lse[i] = log(i + 1)."""
    return torch.zeros(B, Hq, S, D), _randn(gen, B, Hkv, S, D)


FAMILIES = {
    "randn": _fam_randn,
    "needle_diag": _fam_needle_diag,
    "needle_key0": _fam_needle_key0,
    "tempt_next": _fam_tempt_next,
    "rising_max": _fam_rising_max,
    "offset_plus": functools.partial(_fam_offset, 1.0),
    "offset_minus": functools.partial(_fam_offset, -1.0),
    "q_zero": _fam_q_zero,
}


# ---------------------------------------------------------------------------
# float64 reference and the rule's per-element terms (CPU, built once per
# case and never modified)
# ---------------------------------------------------------------------------
def _expand(t, g):
    return t.repeat_interleave(g, 1) if g > 1 else t


def _probs64(q, k, scale):
    """-> (P, lse, s_max) of causal GQA attention on float64 [B, H, S, D]."""
    S = q.shape[2]
    s = (q @ k.transpose(-1, -2)) * scale
    dead = torch.ones(S, S, dtype=torch.bool).triu(1)
    s_max = s.masked_fill(dead, 0.0).abs().amax(-1, keepdim=True)
    s = s.masked_fill(dead, -math.inf)
    lse = torch.logsumexp(s, -1)
    return torch.exp(s - lse[..., None]), lse, s_max


@functools.lru_cache(maxsize=None)
def _case(fam, shape, kind="default"):
    """Inputs, float64 reference and the forward term of one case.

    kind: "default" (scale = D**-0.5), "quarter" (scale = 0.25) or "v3"
    (q pre-multiplied by D**-0.5 * log2e in fp32 and rounded once, as the
    RoPE kernel's oscale does; the reference takes that q with scale ln 2).

    extra_o = 2**-8 * (P @ |V|) + (2*(s_max + 4) + S) * 2**-23 * max|v|.
    First term: every kernel here rounds P to bf16 before the PV MFMA, at
    most 2**-9 relative per term; the factor 2 is the margin for a
    denominator summed from rounded or from unrounded p. Second term: the
    fp32 term of tests/test_paged_attention.py::_case, whose derivation
    carries over unchanged (exp argument and exp, each (s_max + 4) * 2**-23
    relative to p; the S-term fp32 sums of p and p*v; all scaled by max|v|
    of the row's kv head, o being a convex combination of its v).
    """
    B, Hq, Hkv, S = shape
    gen = torch.Generator().manual_seed(
        1000 * sorted(FAMILIES).index(fam) + 97 * B + 13 * Hq + 7 * Hkv + S)
    q, k = FAMILIES[fam](B, Hq, Hkv, S, gen)
    v = _randn(gen, B, Hkv, S, D)
    scale = _f32exact(0.25 if kind == "quarter" else D ** -0.5)
    q, k, v = q.to(BF16).contiguous(), k.to(BF16), v.to(BF16)
    ref_scale = scale
    if kind == "v3":
        q = (q.float() * (scale * ops.LOG2E)).to(BF16)
        ref_scale = ops._LN2
    g = Hq // Hkv
    kx, vx = _expand(_f64(k), g), _expand(_f64(v), g)
    P, lse, s_max = _probs64(_f64(q), kx, ref_scale)
    v_max = vx.abs().amax((2, 3), keepdim=True)
    extra = 2.0 ** -8 * (P @ vx.abs()) \
        + (2 * (s_max + 4) + S) * 2.0 ** -23 * v_max
    return dict(q=q, k=k, v=v, scale=scale, ref_scale=ref_scale, o=P @ vx,
                lse=lse, extra_o=extra, shape=shape, g=g)


def _gout(shape, rows=None):
    """The upstream gradient of a case; rows >= `rows` zeroed if given."""
    B, Hq, Hkv, S = shape
    gen = torch.Generator().manual_seed(31 * S + Hq)
    gout = _randn(gen, B, Hq, S, D).to(BF16)
    if rows is not None:
        gout[:, :, rows:] = 0
    return gout


@functools.lru_cache(maxsize=None)
def _grads(fam, shape, kind="default"):
    """float64 gradients and their first-order terms, per query head.

    With dP = dO @ V^T, Dl = rowsum(dO * O), dS = P * (dP - Dl):
      extra(dv_e) = 2**-8 * (P^T @ |dO|)
      a           = 2**-8 * |dS| + P * 2**-9 * rowsum(|dO| * |O|)
      extra(dq)   = scale * (a @ |K|)
      extra(dk_e) = scale * (a^T @ |Q|)
    from the bf16 rounding of P and dS before the gemms (2**-9 relative
    per term) and the error of Dl computed from bf16 o (2**-9 relative per
    term of the row sum, which enters dS times P), with a margin factor 2
    on the rounding terms.
    """
    c = _case(fam, shape, kind)
    g, scale = c["g"], c["ref_scale"]
    q, kx, vx = _f64(c["q"]), _expand(_f64(c["k"]), g), _expand(_f64(c["v"]), g)
    dO = _f64(_gout(shape))
    P, _, _ = _probs64(q, kx, scale)
    dP = dO @ vx.transpose(-1, -2)
    Dl = (dO * c["o"]).sum(-1, keepdim=True)
    dS = P * (dP - Dl)
    a = 2.0 ** -8 * dS.abs() \
        + P * 2.0 ** -9 * (dO.abs() * c["o"].abs()).sum(-1, keepdim=True)
    return dict(
        dq=scale * (dS @ kx), dk=scale * (dS.transpose(-1, -2) @ q),
        dv=P.transpose(-1, -2) @ dO,
        extra_dq=scale * (a @ kx.abs()),
        extra_dk=scale * (a.transpose(-1, -2) @ q.abs()),
        extra_dv=2.0 ** -8 * (P.transpose(-1, -2) @ dO.abs()))


def _group_sum(t, g):
    B, Hq, S, _ = t.shape
    return t.reshape(B, Hq // g, g, S, D).sum(2)


def _summed_extra(ref_e, extra_e, g):
    """The term of a dk or dv that the project summed over its group.

    g == 1: nothing is summed, the per-head term stands. g > 1: the sum of
    the per-head terms plus 2**-8 * sum|ref_e|. The second part is needed
    because the rule's own 2**-7*|sum| scales with the sum, while each
    addend was rounded to bf16 before the sum and so carries half an ulp of
    its own size (2**-9 relative, with the margin factor 2 of the other
    rounding terms): where the heads of a group cancel, that exceeds any
    multiple of |sum|. Where they do not cancel the hard bound is at most
    1.5 times the sum of the per-head hard bounds."""
    if g == 1:
        return extra_e
    return _group_sum(extra_e + 2.0 ** -8 * ref_e.abs(), g)


def _check_grads(name, c, gr, dq, dk_e=None, dv_e=None, dk=None, dv=None):
    """dq; dk_e / dv_e per query head where the path returns them; dk / dv
    under the group-summed bound where the project did the group sum."""
    g = c["g"]
    _check_ulp(f"{name}_dq", dq, gr["dq"], gr["extra_dq"])
    if dk_e is not None:
        _check_ulp(f"{name}_dk_e", dk_e, gr["dk"], gr["extra_dk"])
        _check_ulp(f"{name}_dv_e", dv_e, gr["dv"], gr["extra_dv"])
    if dk is not None:
        _check_ulp(f"{name}_dk", dk, _group_sum(gr["dk"], g),
                   _summed_extra(gr["dk"], gr["extra_dk"], g))
        _check_ulp(f"{name}_dv", dv, _group_sum(gr["dv"], g),
                   _summed_extra(gr["dv"], gr["extra_dv"], g))


# ---------------------------------------------------------------------------
# Tile-wise emulation of a flash kernel (CPU). leak: key i+1 admitted for
# rows i % T == T-1; drop: the diagonal key dropped for rows i % T == 0,
# i > 0 (row 0 has no other key: dropping it there gives 0/0, which any
# comparison catches and which proves nothing about the bound).
# ---------------------------------------------------------------------------
def _emu_mask(S, j0, T, leak, drop):
    i = torch.arange(S)[:, None]
    j = torch.arange(j0, j0 + T)[None, :]
    mask = j <= i
    if leak:
        mask = mask | ((j == i + 1) & (i % T == T - 1))
    if drop:
        mask = mask & ~((j == i) & (i % T == 0) & (i > 0))
    return mask


def _emu_forward(q, k, v, scale, leak=False, drop=False, T=64):
    B, Hq, S, _ = q.shape
    g = Hq // k.shape[1]
    qf, kf, vf = q.float(), _expand(k.float(), g), _expand(v.float(), g)
    m = torch.full((B, Hq, S), -math.inf)
    l = torch.zeros(B, Hq, S)
    acc = torch.zeros(B, Hq, S, D)
    for j0 in range(0, S, T):
        mask = _emu_mask(S, j0, T, leak, drop)
        s = (qf @ kf[:, :, j0:j0 + T].transpose(-1, -2)) * scale
        s = s.masked_fill(~mask, -math.inf)
        m_new = torch.maximum(m, s.amax(-1))
        shift = m_new.masked_fill(m_new == -math.inf, 0.0)
        p = torch.exp(s - shift[..., None])
        r = torch.exp(m - shift)
        l = l * r + p.sum(-1)
        acc = acc * r[..., None] + p.to(BF16).float() @ vf[:, :, j0:j0 + T]
        m = m_new
    return (acc / l[..., None]).to(BF16), m + torch.log(l)


def _emu_backward(q, k, v, o, lse, gout, scale, leak=False, drop=False, T=64):
    B, Hq, S, _ = q.shape
    g = Hq // k.shape[1]
    qf, kf, vf = q.float(), _expand(k.float(), g), _expand(v.float(), g)
    do = gout.float()
    Dl = (do * o.float()).sum(-1, keepdim=True)
    dq = torch.zeros(B, Hq, S, D)
    dk_e, dv_e = torch.zeros(B, Hq, S, D), torch.zeros(B, Hq, S, D)
    for j0 in range(0, S, T):
        kt, vt = kf[:, :, j0:j0 + T], vf[:, :, j0:j0 + T]
        mask = _emu_mask(S, j0, T, leak, drop)
        s = (qf @ kt.transpose(-1, -2)) * scale
        p = torch.exp(s - lse[..., None]).masked_fill(~mask, 0.0)
        dS = p * (do @ vt.transpose(-1, -2) - Dl)
        pb, dsb = p.to(BF16).float(), dS.to(BF16).float()
        dv_e[:, :, j0:j0 + T] = pb.transpose(-1, -2) @ do
        dk_e[:, :, j0:j0 + T] = (dsb.transpose(-1, -2) @ qf) * scale
        dq += (dsb @ kt) * scale
    return dq.to(BF16), dk_e.to(BF16), dv_e.to(BF16)


# ---------------------------------------------------------------------------
# The families keep their promises (float64 reference alone)
# ---------------------------------------------------------------------------
def test_family_properties():
    B, Hq, Hkv, S = G3
    live = ~torch.ones(S, S, dtype=torch.bool).triu(1)
    for fam in FAMILIES:
        c = _case(fam, G3)
        for key in ("o", "lse", "extra_o"):
            assert bool(c[key].isfinite().all()), f"{fam}: {key} not finite"
        q, kx = _f64(c["q"]), _expand(_f64(c["k"]), c["g"])
        s = (q @ kx.transpose(-1, -2)) * c["scale"]
        P, lse, _ = _probs64(q, kx, c["scale"])
        if fam == "needle_diag":
            assert float(P.diagonal(dim1=-2, dim2=-1).min()) > 1 - 1e-6
        if fam == "needle_key0":
            assert float(P[..., 0].min()) > 1 - 1e-6
        if fam == "tempt_next":
            nxt = s.diagonal(1, -2, -1)                     # s[i, i+1]
            top = s.masked_fill(~live, -math.inf).amax(-1)[..., :-1]
            assert float((nxt - top).min()) > 20
        if fam == "rising_max":  # last row: the tile maxima rise strictly
            tiles = s[:, :, -1].reshape(B, Hq, S // 64, 64).amax(-1)
            assert bool((tiles[..., 1:] > tiles[..., :-1]).all())
        if fam in ("offset_plus", "offset_minus"):
            assert 150 < float(s.abs().min()) and float(s.abs().max()) < 250
            assert float(s.min()) > 0 if fam == "offset_plus" \
                else float(s.max()) < 0
        if fam == "q_zero":
            want = torch.log(torch.arange(1, S + 1, dtype=F64))
            assert float((lse - want).abs().max()) < 1e-12
        if c["g"] > 1 and fam in ("randn", "rising_max", "offset_minus"):
            assert not torch.equal(c["q"][:, 0], c["q"][:, 1])
    for fam in GRAD_FAMILIES:
        gr = _grads(fam, G3)
        assert all(bool(t.isfinite().all()) for t in gr.values()), fam
    c3 = _case("randn", MHA, "v3")  # v3: same softmax, q carries the scale
    c0 = _case("randn", MHA)
    assert float((c3["o"] - c0["o"]).abs().max()) < 2e-2


# ---------------------------------------------------------------------------
# Forward: families x shapes x kernels. The CPU twin is the emulation.
# ---------------------------------------------------------------------------
def _forward(device, kernel, c):
    if device == "cpu":
        return _emu_forward(c["q"], c["k"], c["v"], c["ref_scale"])
    q, k, v = (c[n].to(device) for n in "qkv")
    fn = getattr(ops._ext(), BINDING[kernel])
    if kernel == "v3":
        return fn(q, k, v, c["scale"], prescaled=True)
    return fn(q, k, v, c["scale"])


def _check_forward(device, kernel, fam, shape, kind=None):
    """o and lse under the rules; twice, with identical bits. On "cpu" the
    emulation stands in for the kernel."""
    kind = kind or ("v3" if kernel == "v3" and device != "cpu" else "default")
    c = _case(fam, shape, kind)
    B, Hq, Hkv, S = shape
    tag = "emu" if device == "cpu" else kernel
    name = f"dense_fwd_{tag}_{fam}_{kind}_" + "x".join(map(str, shape))
    o, lse = _forward(device, kernel, c)
    assert o.dtype == BF16 and o.shape == (B, Hq, S, D), name
    assert lse.dtype == F32 and lse.shape == (B, Hq, S), name
    _check_ulp(f"{name}_o", o, c["o"], c["extra_o"])
    _check_lse(f"{name}_lse", lse, c["lse"], S)
    if device != "cpu":
        o2, lse2 = _forward(device, kernel, c)
        assert torch.equal(_bits(o), _bits(o2)), f"{name}: o not deterministic"
        assert torch.equal(_bits(lse), _bits(lse2)), \
            f"{name}: lse not deterministic"


def _check_forward_rule(device, fam):
    """CPU: the emulation passes the rule. GPU: attn_fwd_ck_tr on the same
    case."""
    _check_forward(device, "ck_tr", fam, G3)


_both("dense_forward_rule", _check_forward_rule,
      [(fam,) for fam in FAMILIES])


@pytest.mark.gpu
@pytest.mark.parametrize("fam", list(FAMILIES))
@pytest.mark.parametrize(
    "kernel,shape",
    [(kn, sh) for kn, shapes in KERNEL_SHAPES.items() for sh in shapes
     if (kn, sh) != ("ck_tr", G3)],  # that one is the twin above
    ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_dense_forward_gpu(kernel, shape, fam):
    _check_forward("cuda", kernel, fam, shape)


@pytest.mark.gpu
@pytest.mark.parametrize("fam", ["randn", "rising_max", "tempt_next"])
@pytest.mark.parametrize("kernel", ["ck", "wmma"])
def test_dense_forward_scale_quarter_gpu(kernel, fam):
    """scale = 0.25 instead of D**-0.5."""
    _check_forward("cuda", kernel, fam, G3, kind="quarter")


def test_forward_rule_catches_mask_bugs():
    """The emulation with a one-key leak, or with the diagonal dropped, at
    the 64-key tile edges fails the rule in the family built for it."""
    for fam, bug in (("tempt_next", dict(leak=True)),
                     ("offset_minus", dict(leak=True)),
                     ("needle_diag", dict(drop=True)),
                     ("randn", dict(drop=True)),
                     ("offset_minus", dict(drop=True))):
        c = _case(fam, G3)
        o, lse = _emu_forward(c["q"], c["k"], c["v"], c["scale"], **bug)
        assert bool(o.isfinite().all()) and bool(lse.isfinite().all())
        with pytest.raises(AssertionError, match="beyond one bf16 ulp"):
            assert_bf16_ulp(o, c["o"], c["extra_o"], msg=f"{fam} {bug}")
        with pytest.raises(AssertionError, match="worst got"):
            _check_lse(f"dense_fwd_emu_{fam}_{'_'.join(bug)}_lse", lse,
                       c["lse"], G3[3])


# ---------------------------------------------------------------------------
# Backward: attn_bwd_ck, every pipe. The CPU twin is the emulation.
# ---------------------------------------------------------------------------
def _backward_ck(c, gout, device="cuda"):
    q, k, v = (c[n].to(device) for n in "qkv")
    ext = ops._ext()
    o, lse = ext.attn_fwd_ck_tr(q, k, v, c["scale"])
    return ext.attn_bwd_ck(gout.to(device), q, k, v, o, lse, c["scale"])


def _check_backward(device, pipe, fam, shape):
    """dq, dk_e and dv_e under the gradient rule, with o and lse from
    attn_fwd_ck_tr (the binding does no group sum; the project's is in
    ops.flash_attention, see test_flash_attention_ck_backward_gpu). Run twice: dk_e and dv_e with identical
    bits; dq, an fp32 atomic accumulation, within twice the rule's bound.
    `pipe` is set in the environment by the caller."""
    c, gr = _case(fam, shape), _grads(fam, shape)
    gout = _gout(shape)
    tag = "emu" if device == "cpu" else f"pipe{pipe}"
    name = f"dense_bwd_{tag}_{fam}_" + "x".join(map(str, shape))
    if device == "cpu":
        o, lse = _emu_forward(c["q"], c["k"], c["v"], c["scale"])
        dq, dk_e, dv_e = _emu_backward(c["q"], c["k"], c["v"], o, lse, gout,
                                       c["scale"])
    else:
        dq, dk_e, dv_e = _backward_ck(c, gout)
    for t in (dq, dk_e, dv_e):
        assert t.dtype == BF16 and t.shape == c["q"].shape, name
    _check_grads(name, c, gr, dq, dk_e, dv_e)
    if device != "cpu":
        dq2, dk2, dv2 = _backward_ck(c, gout)
        assert torch.equal(_bits(dk_e), _bits(dk2)), f"{name}: dk_e differs"
        assert torch.equal(_bits(dv_e), _bits(dv2)), f"{name}: dv_e differs"
        diff = (_f64(dq) - _f64(dq2)).abs().cpu()
        twice = 2 * (2.0 ** -7 * gr["dq"].abs() + gr["extra_dq"])
        assert bool((diff <= twice).all()), f"{name}: dq runs disagree"


def test_dense_backward_rule_cpu():
    for fam in GRAD_FAMILIES:
        _check_backward("cpu", None, fam, G3)


@pytest.mark.gpu
@pytest.mark.parametrize("fam", GRAD_FAMILIES)
@pytest.mark.parametrize("shape", [S128, G3, G8],
                         ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("pipe", PIPES, ids=lambda p: f"pipe{p}")
def test_attn_bwd_ck_pipes_gpu(monkeypatch, pipe, shape, fam):
    monkeypatch.setenv("KT_CKBWD_PIPE", str(pipe))
    _check_backward("cuda", pipe, fam, shape)


def test_backward_rule_catches_mask_bugs():
    for fam, bug in (("tempt_next", dict(leak=True)),
                     ("randn", dict(drop=True))):
        c, gr = _case(fam, G3), _grads(fam, G3)
        o, lse = _emu_forward(c["q"], c["k"], c["v"], c["scale"])
        dq, dk_e, dv_e = _emu_backward(c["q"], c["k"], c["v"], o, lse,
                                       _gout(G3), c["scale"], **bug)
        for got, key in ((dq, "dq"), (dk_e, "dk"), (dv_e, "dv")):
            assert bool(got.isfinite().all())
            with pytest.raises(AssertionError, match="beyond one bf16 ulp"):
                assert_bf16_ulp(got, gr[key], gr["extra_" + key],
                                msg=f"{fam} {bug} {key}")


# ---------------------------------------------------------------------------
# A second witness that is not project code: torch's own backward, fed the
# float64-exact o and lse rounded to bf16 / fp32
# ---------------------------------------------------------------------------
def _aten_backward(c, gout, o, lse, scale):
    q = c["q"].cuda()
    kx, vx = _expand(c["k"].cuda(), c["g"]), _expand(c["v"].cuda(), c["g"])
    zero = torch.zeros((), dtype=torch.long, device="cuda")
    dq, dk_e, dv_e, _ = \
        torch.ops.aten._scaled_dot_product_efficient_attention_backward(
            gout.cuda(), q, kx, vx, None, o, lse, zero, zero, 0.0,
            [True, True, True, False], True, scale=scale)
    return dq, dk_e, dv_e


@pytest.mark.gpu
@pytest.mark.parametrize("fam", GRAD_FAMILIES)
@pytest.mark.parametrize("shape", [MHA, G3, G8],
                         ids=lambda s: "x".join(map(str, s)))
def test_aten_backward_witness_gpu(shape, fam):
    c, gr = _case(fam, shape), _grads(fam, shape)
    name = f"dense_bwd_atenwitness_{fam}_" + "x".join(map(str, shape))
    dq, dk_e, dv_e = _aten_backward(
        c, _gout(shape), c["o"].to(BF16).cuda(), c["lse"].to(F32).cuda(),
        c["scale"])
    _check_grads(name, c, gr, dq, dk_e, dv_e)


# ---------------------------------------------------------------------------
# ops.flash_attention: each forward paired with the default (aten) backward
# ---------------------------------------------------------------------------
def _flash(c, impl, gout):
    leaves = [c[n].cuda().requires_grad_(True) for n in "qkv"]
    out = ops.flash_attention(*leaves, scale=c["scale"], impl=impl)
    out.backward(gout.cuda())
    return [out] + [t.grad for t in leaves]


@pytest.mark.gpu
@pytest.mark.parametrize("fam", GRAD_FAMILIES)
@pytest.mark.parametrize("shape", [MHA, G8],
                         ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("impl", ["wmma", "ck", "v3"])
def test_flash_attention_fwd_bwd_gpu(monkeypatch, impl, shape, fam):
    """v3 runs on its contract: prescaled q, effective scale ln 2 for lse
    and the backward; dq is the gradient with respect to that q."""
    monkeypatch.delenv("KT_ATTN_BWD", raising=False)
    kind = "v3" if impl == "v3" else "default"
    c, gr = _case(fam, shape, kind), _grads(fam, shape, kind)
    name = f"dense_flash_{impl}_{fam}_" + "x".join(map(str, shape))
    out, dq, dk, dv = _flash(c, impl, _gout(shape))
    _check_ulp(f"{name}_o", out, c["o"], c["extra_o"])
    assert dk.shape == c["k"].shape and dv.shape == c["v"].shape
    _check_grads(name, c, gr, dq, dk=dk.cpu(), dv=dv.cpu())


@pytest.mark.gpu
@pytest.mark.parametrize("fam", GRAD_FAMILIES)
@pytest.mark.parametrize("shape", [G3, G8],
                         ids=lambda s: "x".join(map(str, s)))
def test_flash_attention_ck_backward_gpu(monkeypatch, shape, fam):
    """KT_ATTN_BWD=ck: attn_bwd_ck (default pipe) behind the ck forward,
    with the group sum of dk_e and dv_e that ops.flash_attention does."""
    monkeypatch.setenv("KT_ATTN_BWD", "ck")
    monkeypatch.delenv("KT_CKBWD_PIPE", raising=False)
    c, gr = _case(fam, shape), _grads(fam, shape)
    name = f"dense_flashckbwd_{fam}_" + "x".join(map(str, shape))
    out, dq, dk, dv = _flash(c, "ck", _gout(shape))
    assert dk.shape == c["k"].shape and dv.shape == c["v"].shape
    _check_grads(name, c, gr, dq, dk=dk.cpu(), dv=dv.cpu())


def test_flash_attention_rejects_unknown_impl():
    q = torch.zeros(1, 2, 256, D, dtype=BF16)
    with pytest.raises(ValueError, match="impl"):
        ops.flash_attention(q, q, q, impl="anything")
    with pytest.raises(ValueError, match="impl"):
        ops.flash_attention(q, q, q, impl="CK")


# ---------------------------------------------------------------------------
# Strides on attn_fwd_ck_tr: three layouts in one call
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_ck_tr_mixed_strides_gpu():
    c = _case("randn", G3)
    B, Hq, Hkv, S = G3
    ext = ops._ext()
    qc, kc, vc = (c[n].cuda() for n in "qkv")
    q = qc.transpose(1, 2).contiguous().transpose(1, 2)  # [B,S,H,D] view
    pad = torch.full((B, Hkv, S, 2 * D), 7.0, dtype=BF16, device="cuda")
    pad[..., :D] = vc
    v = pad[..., :D]                                     # row stride 2*D
    assert not q.is_contiguous() and not v.is_contiguous()
    assert kc.is_contiguous() and v.stride(2) == 2 * D
    o, lse = ext.attn_fwd_ck_tr(q, kc, v, c["scale"])
    oc, lsec = ext.attn_fwd_ck_tr(qc, kc, vc, c["scale"])
    assert o.stride() == q.stride(), "o must come back in q's layout"
    assert torch.equal(_bits(o), _bits(oc)), "o: views != contiguous"
    assert torch.equal(_bits(lse), _bits(lsec)), "lse: views != contiguous"
    _check_ulp("dense_fwd_ck_tr_strided_o", o, c["o"], c["extra_o"])


# ---------------------------------------------------------------------------
# Exact checks
# ---------------------------------------------------------------------------
def _edge_ts(S):
    return [t for t in EDGE_T + [S - 1] if t < S]


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", list(KERNEL_SHAPES))
def test_forward_causality_by_bits_gpu(kernel):
    """Replacing keys and values at rows >= t, with fresh randn or with the
    finite value 2**60, leaves o and lse of rows < t bit-identical.
    tempt_next: the first replaced key is the one row t-1 is aimed at.
    (Never NaN or inf: 0 * NaN in the PV MFMA is NaN in any flash kernel.)"""
    c = dict(_case("tempt_next", MHA, "v3" if kernel == "v3" else "default"))
    S = MHA[3]
    o, lse = _forward("cuda", kernel, c)
    gen = torch.Generator().manual_seed(5)
    for t in _edge_ts(S):
        for fill in ("randn", "big"):
            k2, v2 = c["k"].clone(), c["v"].clone()
            if fill == "randn":
                k2[:, :, t:] = _randn(gen, *k2[:, :, t:].shape).to(BF16)
                v2[:, :, t:] = _randn(gen, *v2[:, :, t:].shape).to(BF16)
            else:
                k2[:, :, t:] = 2.0 ** 60
                v2[:, :, t:] = 2.0 ** 60
            o2, lse2 = _forward("cuda", kernel, dict(c, k=k2, v=v2))
            assert torch.equal(_bits(o[:, :, :t]), _bits(o2[:, :, :t])), \
                f"{kernel}: o of rows < {t} saw keys >= {t} ({fill})"
            assert torch.equal(_bits(lse[:, :, :t]), _bits(lse2[:, :, :t])), \
                f"{kernel}: lse of rows < {t} saw keys >= {t} ({fill})"


def _assert_zero_rows(name, t, dk, dv):
    for label, grad in (("dk", dk), ("dv", dv)):
        tail = grad[:, :, t:]
        assert bool((tail == 0).all()), (
            f"{name}: {label} rows >= {t} not exactly zero, "
            f"{int((tail != 0).sum())} elements")


@pytest.mark.gpu
@pytest.mark.parametrize("pipe", PIPES, ids=lambda p: f"pipe{p}")
def test_attn_bwd_ck_exact_zeros_gpu(monkeypatch, pipe):
    """gout zero on rows >= t: dP, Dl and dS of those rows are exactly zero,
    so dk_e and dv_e of keys >= t are exactly zero; a query row < t that
    leaks onto key t (tempt_next aims it there) makes them non-zero."""
    monkeypatch.setenv("KT_CKBWD_PIPE", str(pipe))
    c = _case("tempt_next", MHA)
    for t in _edge_ts(MHA[3]):
        _, dk_e, dv_e = _backward_ck(c, _gout(MHA, rows=t))
        _assert_zero_rows(f"pipe{pipe}", t, dk_e, dv_e)


@pytest.mark.gpu
@pytest.mark.parametrize("impl", ["wmma", "ck", "v3"])
def test_flash_attention_exact_zeros_gpu(monkeypatch, impl):
    monkeypatch.delenv("KT_ATTN_BWD", raising=False)
    c = _case("tempt_next", MHA, "v3" if impl == "v3" else "default")
    for t in _edge_ts(MHA[3]):
        _, _, dk, dv = _flash(c, impl, _gout(MHA, rows=t))
        _assert_zero_rows(f"flash {impl}", t, dk, dv)


# ---------------------------------------------------------------------------
# Host checks: every bad call raises before an allocation or a launch
# ---------------------------------------------------------------------------
def _t(*shape, dtype=BF16, device="cuda"):
    return torch.zeros(shape, dtype=dtype, device=device)


def _fake_strides(B, H, S, strides):
    """A [B, H, S, 128] view with the given (b, h, s) strides over 128
    elements of storage: a dim with a non-zero stride has size 1, so only
    the batch and head strides can be faked (S = 1 fails the S check)."""
    return _t(D).as_strided((B, H, S, D), strides + (1,))


def _bad_forward_calls(S_ok, bad_S):
    """(label, q, k, v) for one forward binding; S_ok is a length it takes."""
    q, kv = _t(2, 4, S_ok, D), _t(2, 2, S_ok, D)
    calls = [(f"S={s}", _t(2, 4, s, D), _t(2, 2, s, D), _t(2, 2, s, D))
             for s in bad_S]
    calls += [
        ("k dtype", q, kv.half(), kv),
        ("v dtype", q, kv, kv.float()),
        ("q dtype", q.half(), kv, kv),
        ("k other S", q, _t(2, 2, S_ok + 256, D), kv),
        ("k, v other S", q, _t(2, 2, S_ok + 256, D), _t(2, 2, S_ok + 256, D)),
        ("k other B", q, _t(1, 2, S_ok, D), _t(1, 2, S_ok, D)),
        ("k D=64", q, _t(2, 2, S_ok, 64), _t(2, 2, S_ok, 64)),
        ("q D=64", _t(2, 4, S_ok, 64), kv, kv),
        ("Hq % Hkv", q, _t(2, 3, S_ok, D), _t(2, 3, S_ok, D)),
        ("Hkv = 0", q, _t(2, 0, S_ok, D), _t(2, 0, S_ok, D)),
        ("B = 0", _t(0, 4, S_ok, D), _t(0, 2, S_ok, D), _t(0, 2, S_ok, D)),
        ("3-D", q[0], kv[0], kv[0]),
        ("cpu k", q, kv.cpu(), kv),
        ("cpu q", q.cpu(), kv, kv),
        ("k stride(3)", q, _t(2, 2, S_ok, 2 * D)[..., ::2], kv),
        ("q stride(3)", _t(2, 4, S_ok, 2 * D)[..., ::2], kv, kv),
    ]
    return calls


def _assert_all_raise(fn, calls):
    for label, *args in calls:
        with pytest.raises(RuntimeError):
            fn(*args)
            pytest.fail(f"{label}: no error")


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", list(KERNEL_SHAPES))
def test_forward_host_checks_gpu(kernel):
    ext = ops._ext()
    scale = D ** -0.5
    if kernel == "v3":
        def fn(q, k, v):
            return ext.attn_fwd_v3(q, k, v, scale, prescaled=True)
        bad_S = [64, 128, 192, 320, 384]
    else:
        def fn(q, k, v):
            return getattr(ext, BINDING[kernel])(q, k, v, scale)
        bad_S = [64, 192, 320] + ([128] if kernel == "wmma" else [])
    _assert_all_raise(fn, _bad_forward_calls(256, bad_S))
    big = 2 ** 31
    if kernel == "wmma":  # takes contiguous tensors only
        q = _t(2, 256, 4, D).transpose(1, 2)
        with pytest.raises(RuntimeError, match="contiguous"):
            fn(q, _t(2, 2, 256, D), _t(2, 2, 256, D))
        return
    # strides that do not fit ck_tile::index_t, one tensor and one dim at a
    # time; the message names the tensor
    ok = {"q": _t(1, 1, 256, D), "k": _t(1, 1, 256, D), "v": _t(1, 1, 256, D)}
    for name in "qkv":
        for strides in ((big, 0, 0), (0, big, 0), (2 ** 40, 0, 0)):
            args = dict(ok)
            args[name] = _fake_strides(1, 1, 256, strides)
            with pytest.raises(RuntimeError, match=f"{name} stride"):
                fn(args["q"], args["k"], args["v"])
    o, lse = fn(ok["q"], ok["k"], ok["v"])  # the supported form of the call
    assert o.shape == (1, 1, 256, D) and lse.shape == (1, 1, 256)


@pytest.mark.gpu
def test_attn_bwd_ck_host_checks_gpu():
    ext = ops._ext()
    scale = D ** -0.5
    S = 256
    q, kv = _t(2, 4, S, D), _t(2, 2, S, D)
    lse = _t(2, 4, S, dtype=F32)

    def fn(q_, k_, v_, gout=None, o=None, lse_=None):
        gout = torch.zeros_like(q_) if gout is None else gout
        o = torch.zeros_like(q_) if o is None else o
        return ext.attn_bwd_ck(gout, q_, k_, v_, o,
                               lse if lse_ is None else lse_, scale)

    calls = [c for c in _bad_forward_calls(S, [64, 192, 320])
             if not c[0].startswith("S=")]
    _assert_all_raise(fn, calls)
    for s in (64, 192, 320):
        with pytest.raises(RuntimeError):
            ext.attn_bwd_ck(_t(2, 4, s, D), _t(2, 4, s, D), _t(2, 2, s, D),
                            _t(2, 2, s, D), _t(2, 4, s, D),
                            _t(2, 4, s, dtype=F32), scale)
    bad = [
        ("gout other S", dict(gout=_t(2, 4, S + 128, D))),
        ("gout other H", dict(gout=_t(2, 2, S, D))),
        ("gout other B", dict(gout=_t(1, 4, S, D))),
        ("gout dtype", dict(gout=_t(2, 4, S, D, dtype=F32))),
        ("gout cpu", dict(gout=_t(2, 4, S, D, device="cpu"))),
        ("o other S", dict(o=_t(2, 4, S - 128, D))),
        ("o other H", dict(o=_t(2, 8, S, D))),
        ("o dtype", dict(o=_t(2, 4, S, D).half())),
        ("o not contiguous", dict(o=_t(2, S, 4, D).transpose(1, 2))),
        ("lse shape", dict(lse_=_t(2, 4, S + 1, dtype=F32))),
        ("lse dtype", dict(lse_=_t(2, 4, S))),
        ("lse cpu", dict(lse_=_t(2, 4, S, dtype=F32, device="cpu"))),
    ]
    for label, kw in bad:
        with pytest.raises(RuntimeError):
            fn(q, kv, kv, **kw)
            pytest.fail(f"{label}: no error")
    with pytest.raises(RuntimeError):  # k not contiguous
        fn(q, _t(2, S, 2, D).transpose(1, 2), kv)
    dq, dk_e, dv_e = fn(q, kv, kv)  # the supported form of the call
    assert dq.shape == dk_e.shape == dv_e.shape == (2, 4, S, D)
