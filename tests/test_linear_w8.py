"""FP8 weight-only linears: ops.quantize_weight_fp8 / dequantize_weight_fp8,
ops.linear_w8 (the gfx950 skinny-M kernel and its composition fallback),
ops.LinearW8, models.quantize_weights_fp8 / dequantize_weights and the
serving engine on a quantised model.

Contract under test. weight_q is e4m3, weight_scale one power-of-two fp32 per
output row, Wq = float(weight_q) * scale[:, None] is exactly a bf16 matrix,
and y = round(sum_k x * Wq) with fp32 accumulation in any order and one final
rounding. So nothing here needs a tolerance for "fp8 against bf16": the
selection test is exact, and the accuracy bound

    |y - ref| <= 2^-8 |ref| + K 2^-23 (|x| @ |Wq|^T),   ref in float64

is bf16 output rounding plus fp32 accumulation of K terms in any order
(first order (K-1) 2^-24, doubled). It is derived, not measured.

Every op check runs on "cpu" (the composition) and on "cuda" under the gpu
marker, where _linear_w8_kernel_ok is asserted so the kernel cannot silently
be the fallback. Lines starting with "[edges]" report measured errors; run
with -s. Measured on MI355X: worst error / bound 0.965 (accuracy cases, at
N=32 K=128: the output-rounding term) and 0.633 (split-K cases) through the
kernel, and the same two figures through the CPU composition.
"""
import functools

import pytest
import torch

import test_paged_engine as tpe
import test_paged_fp8 as tpf
from kubetorch_amd import models, ops
from kubetorch_amd.models import (BatchedGenerator, Llama,
                                  calibrate_kv_scales, dequantize_weights,
                                  llama_tiny, quantize_weights_fp8)

BF16 = torch.bfloat16
F64 = torch.float64
FP8 = torch.float8_e4m3fn
RAISES = (RuntimeError, ValueError)


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


def _bits(t):
    return t.contiguous().view(torch.int16)


def _is_pow2(s):
    mant, _ = torch.frexp(s)
    return bool(((mant == 0.5) & (s > 0) & s.isfinite()).all())


def _finite_codes():
    codes = torch.arange(256, dtype=torch.uint8)
    finite = codes[codes.view(FP8).float().isfinite()]
    assert finite.numel() == 254
    return finite


def _weights(N, K, seed):
    """(weight_q, weight_scale, Wq float64) on the CPU: randn rows whose
    magnitudes span 2^-6 .. 2^5 around the usual 0.02."""
    gen = torch.Generator().manual_seed(seed)
    mag = 0.02 * 2.0 ** torch.randint(-6, 6, (N, 1), generator=gen).float()
    w = torch.randn(N, K, generator=gen) * mag
    q, s = ops.quantize_weight_fp8(w)
    return q, s, q.double() * s.double()[:, None]


def _bound(x, wq64, ref):
    K = x.shape[-1]
    return 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * (
        x.double().abs() @ wq64.abs().T)


def _ratio(y, x, wq64):
    """max |y - ref| / bound over the outputs, on the CPU in float64."""
    x = x.detach().cpu()
    ref = x.double() @ wq64.T
    err = (y.detach().cpu().double() - ref).abs()
    bound = _bound(x, wq64, ref)
    assert bool(y.isfinite().all())
    # where the bound is 0 the result must be exact
    assert bool((err[bound == 0] == 0).all())
    return float((err / bound.clamp_min(1e-300)).max())


# ---------------------------------------------------------------------------
# 1. The quantiser (CPU)
# ---------------------------------------------------------------------------
def _quantiser_rows():
    gen = torch.Generator().manual_seed(5)
    K = 96
    rows = [torch.randn(K, generator=gen) * 2.0 ** e
            for e in (-30, -14, -7, -3, 0, 4, 11, 25)]
    rows.append(torch.zeros(K))                      # all-zero row
    for e in (-9, 0, 3):                             # amax exactly 448 * 2^e
        r = torch.randn(K, generator=gen).clamp(-1, 1) * 100 * 2.0 ** e
        r[7] = -448.0 * 2.0 ** e
        rows.append(r)
    r = torch.randn(K, generator=gen).clamp(-1, 1)   # amax just above 448*2^e
    r[3] = 449.0 * 2.0 ** -2
    rows.append(r)
    return torch.stack(rows)


def test_quantiser_formula_and_ranges():
    w = _quantiser_rows()
    q, s = ops.quantize_weight_fp8(w)
    assert q.dtype == FP8 and q.shape == w.shape
    assert s.dtype == torch.float32 and s.shape == (w.shape[0],)
    assert _is_pow2(s)
    amax = w.abs().amax(dim=1)
    # the formula, in float64: 2^ceil(log2(amax / 448)); 1.0 for a zero row
    want = torch.where(
        amax == 0, torch.ones(w.shape[0], dtype=F64),
        2.0 ** torch.ceil(torch.log2(amax.double() / 448.0)))
    exact = [9, 10, 11]  # amax / 448 is a power of two: log2 is exact there
    assert torch.equal(s.double()[exact], want[exact])
    assert torch.equal(s.double(), want), (s, want)
    assert float(s[8]) == 1.0
    assert float(s[10]) == 1.0 and float(s[12]) == 0.5
    # the bytes
    want_q = (w.float() * (1 / s)[:, None]).clamp(-448, 448).to(FP8)
    assert torch.equal(q.view(torch.uint8), want_q.view(torch.uint8))
    qa = q.float().abs().amax(dim=1)
    nz = amax > 0
    nz[12] = False
    assert bool(((qa[nz] > 224) & (qa[nz] <= 448)).all()), qa
    # Row 12 is the edge of that range: amax / scale = 224.5 lies in
    # (224, 448] as every row's does, and rounds to the code point 224.
    assert float(amax[12] / s[12]) == 224.5 and float(qa[12]) == 224.0
    assert float(qa[8]) == 0.0
    assert bool((qa[exact] == 448).all())
    # no NaN byte
    assert not bool(((q.view(torch.uint8) & 0x7f) == 0x7f).any())
    # dequantisation is exact, in bf16 too
    exact_wq = q.float() * s[:, None]
    for dt in (BF16, torch.float32, F64):
        d = ops.dequantize_weight_fp8(q, s, dt)
        assert d.dtype == dt
        assert torch.equal(d.float(), exact_wq)
    assert ops.dequantize_weight_fp8(q, s).dtype == BF16
    assert torch.equal(q.to(BF16) * s.to(BF16)[:, None],
                       exact_wq.to(BF16))
    assert torch.equal(exact_wq.to(BF16).float(), exact_wq)


def test_quantiser_accepts_bf16_and_rejects_bad_input():
    w = torch.randn(8, 96).to(BF16)
    q, s = ops.quantize_weight_fp8(w)
    q2, s2 = ops.quantize_weight_fp8(w.float())
    assert torch.equal(q.view(torch.uint8), q2.view(torch.uint8))
    assert torch.equal(s, s2)
    for bad in (torch.randn(8), torch.zeros(4, 4, dtype=torch.int32),
                torch.tensor([[1.0, float("nan")]]),
                torch.tensor([[1.0, float("inf")]])):
        with pytest.raises(RAISES):
            ops.quantize_weight_fp8(bad)


def test_host_validation_rejects_bad_scales():
    q, s = ops.quantize_weight_fp8(torch.randn(4, 128))
    x = torch.randn(2, 128)
    ops.linear_w8(x, q, s)
    for bad in (3.0, 0.0, float("inf"), -1.0, float("nan"), 2.0 ** 41,
                2.0 ** -41):
        sb = s.clone()
        sb[2] = bad
        with pytest.raises(RAISES):
            ops.LinearW8.from_quantized(q, sb)
        with pytest.raises(RAISES):
            ops.linear_w8(x, q, sb)
        with pytest.raises(RAISES):
            ops.dequantize_weight_fp8(q, sb)
    for ok in (2.0 ** 40, 2.0 ** -40):
        sb = s.clone()
        sb[1] = ok
        ops.LinearW8.from_quantized(q, sb)


# ---------------------------------------------------------------------------
# 2. Exact selection, bit for bit
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _selection_weights(N, K):
    """All 254 finite code points over the rows and every k position, mixed
    power-of-two scales 2^-12 .. 2^3."""
    finite = _finite_codes()
    n = torch.arange(N).view(N, 1)
    k = torch.arange(K).view(1, K)
    q = finite[(n * 37 + k * 5 + (k // 128) * 11) % 254].view(FP8)
    s = 2.0 ** ((torch.arange(N) * 7) % 16 - 12).float()
    assert float(s.min()) == 2.0 ** -12 and (N < 16 or float(s.max()) == 8.0)
    assert q.view(torch.uint8).unique().numel() == 254
    wq = (q.float() * s[:, None]).to(BF16)
    assert torch.equal(wq.float(), q.float() * s[:, None])
    return q, s, wq


def _check_selection(device, M, N, K):
    q, s, wq = _selection_weights(N, K)
    qd, sd = q.to(device), s.to(device)
    seen = torch.zeros(K, dtype=torch.bool)
    for base in range(0, K, M):
        km = [(base + m) % K for m in range(M)]
        x = torch.zeros(M, K, dtype=BF16)
        x[torch.arange(M), torch.tensor(km)] = 1.0
        xd = x.to(device)
        if device == "cuda":
            assert ops._linear_w8_kernel_ok(xd, qd, sd)
        y = ops.linear_w8(xd, qd, sd).cpu()
        want = wq[:, km].T.contiguous()  # [M, N]
        assert y.shape == (M, N) and y.dtype == BF16
        # bits, except that an all-zero sum may come out as +0 for -0
        same = _bits(y) == _bits(want)
        zero = (want == 0) & (y == 0)
        assert bool((same | zero).all()), (base, (~(same | zero)).nonzero())
        seen[km] = True
    assert bool(seen.all())  # every residue mod 128, every K tile


_both("selection_exact", _check_selection,
      [(1, 32, 128), (5, 40, 256), (32, 33, 384)])


# ---------------------------------------------------------------------------
# 3. Accuracy against float64
# ---------------------------------------------------------------------------
ACC_M = (1, 3, 16, 17, 32)
ACC_NK = ((32, 128), (1, 128), (40, 256), (512, 256), (256, 512), (1024, 256),
          (64, 14336), (200, 4096))
_worst = {}


def _note(name, device, ratio):
    key = (name, device)
    _worst[key] = max(_worst.get(key, 0.0), ratio)
    print(f"[edges] linear_w8 {name} {device}: error/bound {ratio:.3f} "
          f"(worst so far {_worst[key]:.3f})")


@functools.lru_cache(maxsize=None)
def _acc_weights(N, K):
    return _weights(N, K, seed=1000 * N + K)


def _acc_inputs(M, K, seed):
    """randn rows, and the same with the last row at magnitudes up to 2^8."""
    gen = torch.Generator().manual_seed(seed)
    xa = torch.randn(M, K, generator=gen).to(BF16)
    xb = xa.clone()
    xb[M - 1] = ((torch.rand(K, generator=gen) * 2 - 1) * 256.0).to(BF16)
    return xa, xb


def _check_accuracy(device, N, K):
    q, s, wq64 = _acc_weights(N, K)
    qd, sd = q.to(device), s.to(device)
    worst = 0.0
    for M in ACC_M:
        for x in _acc_inputs(M, K, seed=M):
            xd = x.to(device)
            if device == "cuda":
                assert ops._linear_w8_kernel_ok(xd, qd, sd)
            y = ops.linear_w8(xd, qd, sd)
            assert y.shape == (M, N) and y.dtype == BF16
            worst = max(worst, _ratio(y, x, wq64))
    _note(f"accuracy N={N} K={K}", device, worst)
    assert worst <= 1.0, worst


_both("accuracy_f64", _check_accuracy, list(ACC_NK))


def test_leading_dimensions_flatten():
    q, s, wq64 = _acc_weights(40, 256)
    x = torch.randn(2, 3, 256).to(BF16)
    y = ops.linear_w8(x, q, s)
    assert y.shape == (2, 3, 40)
    assert torch.equal(y.view(6, 40), ops.linear_w8(x.view(6, 256), q, s))
    assert ops.linear_w8(x[0, 0], q, s).shape == (40,)
    assert ops.linear_w8(x[:0], q, s).shape == (0, 3, 40)


# ---------------------------------------------------------------------------
# 4. Split-K
# ---------------------------------------------------------------------------
def _check_splits(device, M, N, K):
    q, s, wq64 = _weights(N, K, seed=77)
    qd, sd = q.to(device), s.to(device)
    x = _acc_inputs(M, K, seed=9)[1]
    xd = x.to(device)
    worst = 0.0
    for S in (1, 2, 3, 8):
        y1 = ops.linear_w8(xd, qd, sd, num_splits=S)
        y2 = ops.linear_w8(xd, qd, sd, num_splits=S)
        assert torch.equal(_bits(y1), _bits(y2)), S
        worst = max(worst, _ratio(y1, x, wq64))
    _note(f"split-K M={M} N={N} K={K}", device, worst)
    assert worst <= 1.0, worst
    with pytest.raises(RAISES):
        ops.linear_w8(xd, qd, sd, num_splits=0)
    with pytest.raises(RAISES):
        ops.linear_w8(xd, qd, sd, num_splits=65)


_both("split_k", _check_splits, [(8, 128, 2048), (32, 48, 1152)])


@pytest.mark.gpu
def test_split_choice_depends_on_shape_only_gpu():
    """The 8B shapes all get a grid of at least one workgroup per CU."""
    for N, K in ((6144, 4096), (4096, 4096), (28672, 4096), (4096, 14336),
                 (128256, 4096)):
        S = ops.linear_w8_splits(N, K)
        assert 1 <= S <= 8
        assert -(-N // 128) * S >= 256, (N, K, S)
        assert K // 128 // S >= 4  # slices stay at least four tiles long


# ---------------------------------------------------------------------------
# 5. Batch invariance, strides, the dispatch predicate (GPU)
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("N,K", [(200, 4096), (40, 256)])
def test_batch_invariance_gpu(N, K):
    """Row m of an M = 32 call equals the M = 1 call on that row alone."""
    q, s, _ = _acc_weights(N, K)
    qd, sd = q.cuda(), s.cuda()
    x = _acc_inputs(32, K, seed=4)[1].cuda()
    assert ops._linear_w8_kernel_ok(x, qd, sd)
    y = ops.linear_w8(x, qd, sd)
    for m in range(32):
        assert ops._linear_w8_kernel_ok(x[m:m + 1], qd, sd)
        ym = ops.linear_w8(x[m:m + 1], qd, sd)
        assert torch.equal(_bits(ym[0]), _bits(y[m])), m


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 5, 32])
def test_rows_past_m_are_not_read_gpu(M):
    N, K = 40, 256
    q, s, wq64 = _acc_weights(N, K)
    qd, sd = q.cuda(), s.cuda()
    x = _acc_inputs(M, K, seed=6)[0]
    xbig = torch.full((M + 7, K), float("nan"), dtype=BF16, device="cuda")
    xbig[:M] = x.cuda()
    assert ops._linear_w8_kernel_ok(xbig[:M], qd, sd)
    y = ops.linear_w8(xbig[:M], qd, sd)
    assert not bool(y.isnan().any())
    assert torch.equal(_bits(y), _bits(ops.linear_w8(x.cuda(), qd, sd)))
    assert _ratio(y, x, wq64) <= 1.0


@pytest.mark.gpu
def test_strided_x_gpu():
    N, K, M = 40, 256, 5
    q, s, wq64 = _acc_weights(N, K)
    qd, sd = q.cuda(), s.cuda()
    x = _acc_inputs(M, K, seed=8)[0]
    want = ops.linear_w8(x.cuda(), qd, sd)
    wide = torch.full((M, 3 * K), float("nan"), dtype=BF16, device="cuda")
    # a column slice, row stride 3K: 16-byte aligned, the kernel takes it
    wide[:, K:2 * K] = x.cuda()
    xs = wide[:, K:2 * K]
    assert xs.stride(0) == 3 * K and ops._linear_w8_kernel_ok(xs, qd, sd)
    assert torch.equal(_bits(ops.linear_w8(xs, qd, sd)), _bits(want))
    # the same slice 4 elements (8 bytes) off alignment: the composition
    wide.fill_(float("nan"))
    wide[:, 4:4 + K] = x.cuda()
    xs = wide[:, 4:4 + K]
    assert not ops._linear_w8_kernel_ok(xs, qd, sd)
    assert _ratio(ops.linear_w8(xs, qd, sd), x, wq64) <= 1.0
    # a [B, 1, K] decode activation and a 3-D view with strided rows
    x3 = x.cuda().view(M, 1, K)
    assert ops._linear_w8_kernel_ok(x3, qd, sd)
    assert torch.equal(_bits(ops.linear_w8(x3, qd, sd).view(M, N)),
                       _bits(want))


@pytest.mark.gpu
def test_predicate_false_inputs_are_still_correct_gpu():
    q, s, wq64 = _acc_weights(40, 256)
    qd, sd = q.cuda(), s.cuda()
    # M = 33
    x = _acc_inputs(33, 256, seed=1)[0]
    assert not ops._linear_w8_kernel_ok(x.cuda(), qd, sd)
    assert _ratio(ops.linear_w8(x.cuda(), qd, sd), x, wq64) <= 1.0
    # fp32 x (the bound's output-rounding term is then generous)
    x = _acc_inputs(4, 256, seed=2)[0].float()
    assert not ops._linear_w8_kernel_ok(x.cuda(), qd, sd)
    y = ops.linear_w8(x.cuda(), qd, sd)
    assert y.dtype == torch.float32 and _ratio(y, x, wq64) <= 1.0
    # a last-dim stride of 4 elements
    xw = torch.zeros(4, 4 * 256, dtype=BF16)
    xw[:, ::4] = _acc_inputs(4, 256, seed=3)[0]
    xs = xw.cuda()[:, ::4]
    assert xs.stride(1) == 4 and not ops._linear_w8_kernel_ok(xs, qd, sd)
    assert _ratio(ops.linear_w8(xs, qd, sd), xw[:, ::4], wq64) <= 1.0
    # K = 192
    q2, s2, wq2 = _weights(40, 192, seed=12)
    x = _acc_inputs(4, 192, seed=5)[0]
    assert not ops._linear_w8_kernel_ok(x.cuda(), q2.cuda(), s2.cuda())
    assert _ratio(ops.linear_w8(x.cuda(), q2.cuda(), s2.cuda()), x,
                  wq2) <= 1.0
    # a transposed (non-contiguous) weight_q
    qt = q.t().contiguous().t().cuda()
    x = _acc_inputs(4, 256, seed=7)[0]
    assert not qt.is_contiguous()
    assert not ops._linear_w8_kernel_ok(x.cuda(), qt, sd)
    assert _ratio(ops.linear_w8(x.cuda(), qt, sd), x, wq64) <= 1.0


# ---------------------------------------------------------------------------
# 6. Errors
# ---------------------------------------------------------------------------
def _check_errors(device):
    q, s, _ = _acc_weights(40, 256)
    q, s = q.to(device), s.to(device)
    x = torch.randn(3, 256).to(BF16).to(device)
    ops.linear_w8(x, q, s)
    for name in ("float8_e4m3fnuz", "float8_e5m2", "float8_e5m2fnuz"):
        bad = torch.zeros(40, 256, device=device).to(getattr(torch, name))
        with pytest.raises(RAISES):
            ops.linear_w8(x, bad, s)
    with pytest.raises(RAISES):
        ops.linear_w8(x, q.to(BF16), s)           # unquantised weight
    with pytest.raises(RAISES):
        ops.linear_w8(x, q, s.to(BF16))           # bf16 scale
    with pytest.raises(RAISES):
        ops.linear_w8(x, q, s[:39])               # wrong length
    with pytest.raises(RAISES):
        ops.linear_w8(x, q, s.view(40, 1))
    with pytest.raises(RAISES):
        ops.linear_w8(x[:, :128], q, s)           # last dim is not K
    with pytest.raises(RAISES):
        ops.linear_w8(x, q[0], s)                 # 1-D weight
    with pytest.raises(RAISES):
        ops.linear_w8(x.to(torch.int32), q, s)
    # devices
    with pytest.raises(RAISES):
        ops.linear_w8(x.to("meta"), q, s)
    with pytest.raises(RAISES):
        ops.linear_w8(x, q, s.to("meta"))
    if device == "cuda":
        with pytest.raises(RAISES):
            ops.linear_w8(x.cpu(), q, s)
        with pytest.raises(RAISES):
            ops.linear_w8(x, q.cpu(), s.cpu())
    # inference only
    xg = x.clone().requires_grad_(True)
    with pytest.raises(RuntimeError):
        ops.linear_w8(xg, q, s)
    with torch.no_grad():
        ops.linear_w8(xg, q, s)


_both("errors", _check_errors)


# ---------------------------------------------------------------------------
# 7. Module and model (CPU)
# ---------------------------------------------------------------------------
def _tiny(seed=21, **kw):
    torch.manual_seed(seed)
    return Llama(llama_tiny(**kw)).eval()


def _linears(model, kind):
    return {n: m for n, m in model.named_modules() if isinstance(m, kind)}


def test_linear_w8_module():
    with pytest.raises(RAISES):
        ops.LinearW8.from_linear(torch.nn.Linear(128, 8, bias=True))
    lin = ops.Linear(128, 8)
    mod = ops.LinearW8.from_linear(lin)
    assert (mod.in_features, mod.out_features) == (128, 8)
    sd = mod.state_dict()
    assert sorted(sd) == ["weight_q", "weight_scale"]
    assert sd["weight_q"].dtype == FP8 and sd["weight_q"].shape == (8, 128)
    assert sd["weight_scale"].dtype == torch.float32
    assert not list(mod.parameters())
    fresh = ops.LinearW8(128, 8)
    assert not torch.equal(fresh.weight_q.view(torch.uint8),
                           mod.weight_q.view(torch.uint8))
    fresh.load_state_dict(sd)
    assert torch.equal(fresh.weight_q.view(torch.uint8),
                       mod.weight_q.view(torch.uint8))
    assert torch.equal(fresh.weight_scale, mod.weight_scale)
    x = torch.randn(3, 128)
    want = torch.nn.functional.linear(
        x, ops.dequantize_weight_fp8(mod.weight_q, mod.weight_scale,
                                     torch.float32))
    assert torch.equal(mod(x), want) and torch.equal(fresh(x), want)
    # a dtype cast of the module leaves the bytes and the fp32 scale alone
    cast = ops.LinearW8.from_linear(lin).to(BF16)
    assert cast.weight_q.dtype == FP8
    assert cast.weight_scale.dtype == torch.float32
    assert torch.equal(cast.weight_q.view(torch.uint8),
                       mod.weight_q.view(torch.uint8))


def test_quantize_weights_fp8_model():
    model = _tiny()
    cfg = model.cfg
    n_lin = 4 * cfg.n_layers + 1
    before = {n: m.weight.clone()
              for n, m in _linears(model, ops.Linear).items()}
    assert len(before) == n_lin
    qm = quantize_weights_fp8(model)
    assert qm is not model
    # the input model is untouched
    after = _linears(model, ops.Linear)
    assert sorted(after) == sorted(before)
    assert all(torch.equal(after[n].weight, before[n]) for n in before)
    # exactly the ops.Linear layers are replaced, nothing else
    w8 = _linears(qm, ops.LinearW8)
    assert sorted(w8) == sorted(before) and len(w8) == n_lin
    assert not _linears(qm, ops.Linear)
    assert sorted(n.split(".")[-1] for n in w8) == sorted(
        ["wqkv", "wo", "w_gate_up", "w_down"] * cfg.n_layers + ["lm_head"])
    assert torch.equal(qm.embed.weight, model.embed.weight)
    for n, m in w8.items():
        out_f, in_f = before[n].shape
        q, s = ops.quantize_weight_fp8(before[n])
        assert torch.equal(m.weight_q.view(torch.uint8), q.view(torch.uint8))
        assert torch.equal(m.weight_scale, s)
        # one byte per element plus four per row
        nbytes = sum(b.numel() * b.element_size() for b in m.buffers())
        assert nbytes == out_f * in_f + 4 * out_f
    # skip
    qs = quantize_weights_fp8(model, skip=("lm_head",))
    assert isinstance(qs.lm_head, ops.Linear)
    assert len(_linears(qs, ops.LinearW8)) == n_lin - 1
    qs = quantize_weights_fp8(model, skip=("w_down", "layers.0.attn.wo"))
    assert len(_linears(qs, ops.LinearW8)) == n_lin - cfg.n_layers - 1
    assert isinstance(qs.layers[1].attn.wo, ops.LinearW8)
    # in place: the same object, no ops.Linear weight left behind
    m2 = copy_of = _tiny()
    old = list(_linears(m2, ops.Linear).values())
    assert quantize_weights_fp8(m2, inplace=True) is copy_of
    assert not _linears(m2, ops.Linear)
    assert all(m.weight is None for m in old)
    assert len(_linears(m2, ops.LinearW8)) == n_lin
    # state_dict round trip of the whole model
    m3 = quantize_weights_fp8(_tiny(seed=22))
    m3.load_state_dict(qm.state_dict())
    for n, m in _linears(m3, ops.LinearW8).items():
        assert torch.equal(m.weight_q.view(torch.uint8),
                           w8[n].weight_q.view(torch.uint8))


def test_quantize_weights_leaves_moe_experts_alone():
    model = models.convert_to_moe(_tiny(), n_experts=4, top_k=2)
    plain = {n for n, m in model.named_modules()
             if type(m) is torch.nn.Linear}
    assert plain
    qm = quantize_weights_fp8(model)
    assert {n for n, m in qm.named_modules()
            if type(m) is torch.nn.Linear} == plain
    assert not _linears(qm, ops.Linear)


def test_dequantize_weights_model():
    model = _tiny()
    qm = quantize_weights_fp8(model)
    dm = dequantize_weights(qm)
    assert dm is not qm and _linears(qm, ops.LinearW8)  # qm unchanged
    assert not _linears(dm, ops.LinearW8)
    lin = _linears(dm, ops.Linear)
    w8 = _linears(qm, ops.LinearW8)
    assert sorted(lin) == sorted(w8)
    for n, m in lin.items():
        wq = w8[n].weight_q.float() * w8[n].weight_scale[:, None]
        assert m.weight.dtype == model.embed.weight.dtype
        assert torch.equal(m.weight.float(), wq)
    bf = dequantize_weights(qm, dtype=BF16)
    assert all(m.weight.dtype == BF16
               for m in _linears(bf, ops.Linear).values())
    assert all(torch.equal(m.weight.float(), lin[n].weight.float())
               for n, m in _linears(bf, ops.Linear).items())
    # quantising the dequantised model represents the same matrix again (a
    # row whose largest byte had rounded down to 224 gets half the scale and
    # twice the bytes)
    again = quantize_weights_fp8(dm)
    for n, m in _linears(again, ops.LinearW8).items():
        assert torch.equal(
            ops.dequantize_weight_fp8(m.weight_q, m.weight_scale),
            ops.dequantize_weight_fp8(w8[n].weight_q, w8[n].weight_scale))


# ---------------------------------------------------------------------------
# 8. Engine (CPU), token for token
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cpu_pair():
    qm = quantize_weights_fp8(_tiny(seed=33))
    return qm, dequantize_weights(qm)


def _staggered(model, prompts, new=10, **kw):
    eng = BatchedGenerator(model, max_batch=3, max_len=64, **kw)
    rids = [eng.submit(p, max_new_tokens=new) for p in prompts[:2]]
    for _ in range(3):  # staggered join
        eng.step()
    rids += [eng.submit(p, max_new_tokens=new) for p in prompts[2:]]
    out = eng.run()
    return [out[r] for r in rids]


@pytest.mark.parametrize("kw", [
    dict(kv="slot"), dict(kv="paged", page_size=16),
    dict(kv="paged", page_size=16, prefill="paged")],
    ids=["slot", "paged", "paged-prefill"])
def test_engine_matches_dequantised_model_cpu(kw):
    """The CPU path is F.linear on the same matrix in both models."""
    qm, dm = _cpu_pair()
    prompts = tpf._cpu_prompts(qm.cfg)
    got = _staggered(qm, prompts, **kw)
    want = _staggered(dm, prompts, **kw)
    assert got == want
    assert all(len(t) == len(p) + 10 for p, t in zip(prompts, got))


def test_generate_matches_dequantised_model_cpu():
    qm, dm = _cpu_pair()
    toks = torch.tensor([tpf._cpu_prompts(qm.cfg)[0]])
    assert torch.equal(qm.generate(toks, 8), dm.generate(toks, 8))
    with torch.no_grad():
        assert torch.equal(qm(toks), dm(toks))


# ---------------------------------------------------------------------------
# 9. Engine (GPU)
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_pair():
    cfg = llama_tiny(max_seq_len=192)
    torch.manual_seed(11)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(BF16)
    try:
        with torch.device("cuda"):
            model = Llama(cfg).eval()
    finally:
        torch.set_default_dtype(prev)
    qm = quantize_weights_fp8(model, inplace=True)
    assert all(m.weight_q.is_cuda for m in _linears(qm, ops.LinearW8).values())
    dm = dequantize_weights(qm)
    assert all(m.weight.dtype == BF16 and m.weight.is_cuda
               for m in _linears(dm, ops.Linear).values())
    return qm, dm


def _gpu_run(model, prompts, graph, new=12, max_len=96, **kw):
    eng = BatchedGenerator(model, max_batch=3, max_len=max_len, graph=graph,
                           **kw)
    rids = [eng.submit(p, max_new_tokens=new) for p in prompts[:2]]
    for _ in range(3):  # staggered join
        eng.step()
    rids += [eng.submit(p, max_new_tokens=new) for p in prompts[2:]]
    out = eng.run()
    return eng, [out[r] for r in rids]


def _count_kernel_calls(monkeypatch):
    """Count ops.linear_w8 calls that the kernel takes."""
    calls = {"kernel": 0, "fallback": 0}
    real = ops._linear_w8_kernel_ok

    def spy(x, q, s):
        ok = real(x, q, s)
        calls["kernel" if ok else "fallback"] += 1
        return ok
    monkeypatch.setattr(ops, "_linear_w8_kernel_ok", spy)
    return calls


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_w8_paged_decode_graph_matches_eager_gpu(gpu_pair, monkeypatch):
    qm, dm = gpu_pair
    prompts = tpe._gpu_prompts(qm.cfg)
    calls = _count_kernel_calls(monkeypatch)
    kw = dict(kv="paged", page_size=16)
    _, eager = _gpu_run(qm, prompts, False, **kw)
    assert calls["kernel"] > 0  # decode steps run the kernel
    eng, graphed = _gpu_run(qm, prompts, True, **kw)
    assert eager == graphed
    assert eng._use_graph and len(eng._graphs) == 1
    assert eng._pkv.free_pages == eng._pkv.num_pages
    for p, toks in zip(prompts, graphed):
        assert len(toks) == len(p) + 12
        tpe._assert_teacher_forced(dm, len(p), toks)


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_w8_slot_decode_graph_matches_eager_gpu(gpu_pair):
    """max_len 160 with one prompt that crosses a horizon of 128: the slot
    engine uses the buckets 128 and 160 and captures one graph for each."""
    qm, dm = gpu_pair
    prompts = tpe._gpu_prompts(qm.cfg)
    gen = torch.Generator().manual_seed(5)
    prompts[2] = torch.randint(0, qm.cfg.vocab_size, (120,),
                               generator=gen).tolist()
    kw = dict(kv="slot", max_len=160)
    _, eager = _gpu_run(qm, prompts, False, **kw)
    eng, graphed = _gpu_run(qm, prompts, True, **kw)
    assert eager == graphed
    assert eng._use_graph and sorted(eng._graphs) == [128, 160]
    for p, toks in zip(prompts, graphed):
        assert len(toks) == len(p) + 12
        tpe._assert_teacher_forced(dm, len(p), toks)


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_w8_composes_with_fp8_pages_and_fused_sampler_gpu(gpu_pair):
    """kv_dtype="fp8", sampler="fused", prefix cache and paged prefill on a
    quantised model: graph and eager agree, greedy tokens pass the gross
    check."""
    qm, dm = gpu_pair
    prompts = tpe._gpu_prompts(qm.cfg)
    kw = dict(kv="paged", page_size=16, kv_dtype="fp8", sampler="fused",
              prefix_cache=True,
              kv_scales=calibrate_kv_scales(dm, prompts[2], margin=1.5))
    _, eager = _gpu_run(qm, prompts, False, **kw)
    eng, graphed = _gpu_run(qm, prompts, True, **kw)
    assert eager == graphed
    assert eng._use_graph and len(eng._graphs) == 1
    for p, toks in zip(prompts, graphed):
        assert len(toks) == len(p) + 12
        tpe._assert_teacher_forced(dm, len(p), toks)


# ---------------------------------------------------------------------------
# bench_decode.py --weight-dtype
# ---------------------------------------------------------------------------
def test_bench_decode_weight_dtype_flag(monkeypatch, capsys):
    """fp8 quantises the built model and says so in the JSON line; the
    default prints the keys it printed before."""
    import importlib.util
    import json
    import os
    import sys

    path = os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "bench_decode.py")
    spec = importlib.util.spec_from_file_location("bench_decode", path)
    bd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bd)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    base = ["bench_decode.py", "--model", "tiny", "--batch", "2", "--prompt",
            "8", "--new", "4", "--kv", "paged"]
    built = []
    real = bd.make_engine
    monkeypatch.setattr(bd, "make_engine", lambda model, *a, **kw: (
        built.append(model), real(model, *a, **kw))[1])
    out = {}
    for mode in ("bf16", "fp8"):
        monkeypatch.setattr(sys, "argv", base + ["--weight-dtype", mode])
        bd.main()
        line = capsys.readouterr().out.strip().splitlines()[-1]
        out[mode] = json.loads(line)
        n_w8 = len(_linears(built[-1], ops.LinearW8))
        assert n_w8 == (0 if mode == "bf16" else 4 * 2 + 1)
    assert "weight_dtype" not in out["bf16"]
    assert out["fp8"]["weight_dtype"] == "fp8"
    assert set(out["fp8"]) - set(out["bf16"]) == {"weight_dtype"}
    monkeypatch.setattr(sys, "argv", base[:-2])
    bd.main()
    default = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "weight_dtype" not in default and default["kv"] == "slot"
