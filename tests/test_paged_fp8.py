"""FP8 (OCP e4m3) paged KV cache: the quantising ops.paged_kv_write,
ops.paged_attention_decode / ops.paged_attention_prefill over fp8 pools,
PagedKVCache / BatchedGenerator(kv_dtype="fp8") and calibrate_kv_scales.

Same scheme as tests/test_paged_attention.py and tests/test_paged_prefill.py,
whose cases, references and bounds are reused: every op check runs on "cpu"
against the project's reference path and on "cuda" under the gpu marker,
where it runs the gfx950 kernels.

Contract under test. A pool byte encodes x / scale with a static fp32 scale
per kv head; it is written as
(x.float() * scale.reciprocal()).clamp(-448, 448).to(float8_e4m3fn), which
the kernel must reproduce bit for bit, and read back as float(byte) * scale.
e4m3 -> fp32 is exact, so against the dequantised contents of its own pool a
read kernel does the arithmetic of the bf16 kernel: the attention checks use
the bf16 files' bounds unchanged, with s_max and v_max taken from the
dequantised values.

Lines starting with "[edges]" report measured errors; run with -s.
"""
import functools

import pytest
import torch

import test_paged_attention as tpa
import test_paged_engine as tpe
import test_paged_prefill as tpp
from kubetorch_amd import ops
from kubetorch_amd.models import (BatchedGenerator, Llama, PagedKVCache,
                                  calibrate_kv_scales, llama_tiny)

BF16 = torch.bfloat16
F64 = torch.float64
FP8 = torch.float8_e4m3fn
RAISES = (RuntimeError, ValueError)

# (hd, Hq, Hkv): hd {64, 128} x group {1, 4, 8}, and llama_tiny's group 2
CONFIGS = [(64, 4, 4), (64, 8, 2), (64, 8, 1), (128, 8, 8), (128, 8, 2),
           (128, 8, 1), (64, 4, 2)]
CASES = [c + (ps,) for c in CONFIGS for ps in (16, 64)]

_f64, _bits, _note = tpa._f64, tpa._bits, tpa._note


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


def _quant(x, scale):
    """The contract's reference, on the CPU: x [..., n_kv, hd] (or a pool
    [P, n_kv, ps, hd] with scale viewed to match) -> e4m3."""
    return (x.float() * scale.reciprocal()).clamp(-448, 448).to(FP8)


def _scales(Hkv, seed):
    """Non-trivial, non-power-of-two per-head scales that put randn data in
    the upper binades of e4m3."""
    gen = torch.Generator().manual_seed(seed)
    return ((0.011 + 0.02 * torch.rand(Hkv, generator=gen)).float(),
            (0.013 + 0.02 * torch.rand(Hkv, generator=gen)).float())


def _fp8_pools(c, Hkv, seed):
    """fp8 pools quantised from a bf16 case's pools, their scales, and the
    dequantised float64 contents float64(byte) * scale."""
    ks, vs = _scales(Hkv, seed)
    kq = _quant(c["kp"], ks.view(1, Hkv, 1, 1))
    vq = _quant(c["vp"], vs.view(1, Hkv, 1, 1))
    kd = _f64(kq.float()) * _f64(ks).view(1, Hkv, 1, 1)
    vd = _f64(vq.float()) * _f64(vs).view(1, Hkv, 1, 1)
    return dict(kq=kq, vq=vq, ks=ks, vs=vs, kd=kd, vd=vd)


def _poison(pool, valid, byte):
    """`byte` at every position that holds no valid token."""
    dead = ~valid[:, None, :, None]
    b = pool.view(torch.uint8)
    return torch.where(dead, torch.tensor(byte, dtype=torch.uint8), b).view(FP8)


# ---------------------------------------------------------------------------
# 1. paged_kv_write into fp8 pools: bitwise
# ---------------------------------------------------------------------------
def _e4m3_probe_values():
    """As bf16: all 254 finite code points (with +-0), every midpoint of two
    adjacent code points (ties; 2^-10 -> 0 among them), values in (448, 480),
    +-inf and NaN."""
    codes = torch.arange(256, dtype=torch.uint8).view(FP8).float()
    finite = codes[codes.isfinite()]
    assert finite.numel() == 254
    pos = finite[finite >= 0].unique()          # 0 .. 448, 127 values
    assert pos.numel() == 127 and float(pos[-1]) == 448.0
    mid = (pos[:-1] + pos[1:]) / 2
    assert float(mid[0]) == 2.0 ** -10
    extra = torch.tensor([450.0, 464.0, 478.0, -450.0, -478.0, float("inf"),
                          float("-inf"), float("nan")])
    vals = torch.cat([finite, mid, -mid, extra])
    assert torch.equal(vals.to(BF16).float().nan_to_num(7.0),
                       vals.nan_to_num(7.0)), "not representable in bf16"
    return vals.to(BF16)


def _sentinel_bytes(shape):
    n = 1
    for s in shape:
        n *= s
    return ((torch.arange(n, dtype=torch.int64) * 7 + 3) % 251) \
        .to(torch.uint8).reshape(shape)


def _check_write(device, hd, scaled):
    T, Hkv, Hq, ps, P = 5, 2, 4, 16, 4
    vals = _e4m3_probe_values()
    # negative, past the pool, two pages, last offset of a page
    sm = torch.tensor([-1, P * ps + 3, 1 * ps + 5, 3 * ps + 0, 3 * ps + 15],
                      dtype=torch.int32)
    written = [2, 3, 4]
    n = len(written) * Hkv * hd
    assert 2 * n >= vals.numel()
    cyc = vals.repeat(-(-2 * n // vals.numel()))[:2 * n]
    gen = torch.Generator().manual_seed(hd)
    # k/v as the qkv split gives them: strided views of a wider row
    wide = torch.randn(T, (Hq + 2 * Hkv) * hd, generator=gen).to(BF16)
    k_new = wide[:, Hq * hd:(Hq + Hkv) * hd].view(T, Hkv, hd)
    v_new = wide[:, (Hq + Hkv) * hd:].view(T, Hkv, hd)
    k_new[written] = cyc[:n].view(len(written), Hkv, hd)
    v_new[written] = cyc[n:].view(len(written), Hkv, hd)
    if scaled:
        ks = torch.tensor([0.37, 2.9])
        vs = torch.tensor([1.7, 0.081])
    else:
        ks = vs = None
    one = torch.ones(Hkv)
    shape = (P, Hkv, ps, hd)
    ref_k = _sentinel_bytes(shape).view(FP8)
    ref_v = (255 - _sentinel_bytes(shape)).view(FP8)
    kp, vp = ref_k.clone().to(device), ref_v.clone().to(device)
    page, off = torch.tensor([1, 3, 3]), torch.tensor([5, 0, 15])
    ref_k[page, :, off] = _quant(k_new[written],
                                 (one if ks is None else ks).view(1, Hkv, 1))
    ref_v[page, :, off] = _quant(v_new[written],
                                 (one if vs is None else vs).view(1, Hkv, 1))
    wd = wide.to(device)
    kd = wd[:, Hq * hd:(Hq + Hkv) * hd].view(T, Hkv, hd)
    vd = wd[:, (Hq + Hkv) * hd:].view(T, Hkv, hd)
    assert not kd.is_contiguous()
    ops.paged_kv_write(kd, vd, kp, vp, sm.to(device),
                       None if ks is None else ks.to(device),
                       None if vs is None else vs.to(device))
    for name, got, ref in (("k", kp, ref_k), ("v", vp, ref_v)):
        g = got.cpu().view(torch.uint8).reshape(-1)
        r = ref.view(torch.uint8).reshape(-1)
        nan = (r & 0x7f) == 0x7f
        assert bool(((g[nan] & 0x7f) == 0x7f).all()), f"{name}: NaN lost"
        bad = (g != r) & ~nan
        if bool(bad.any()):
            i = int(bad.nonzero()[0])
            raise AssertionError(
                f"{name} pool: {int(bad.sum())} bytes differ; first at {i}: "
                f"got {int(g[i]):#x}, reference {int(r[i]):#x}")
    if not scaled:  # the probe values did what they are there for
        rk = ref_k[page, :, off].view(torch.uint8)
        rv = ref_v[page, :, off].view(torch.uint8)
        seen = set(rk.reshape(-1).tolist()) | set(rv.reshape(-1).tolist())
        assert seen >= set(range(256)) - {0x7f, 0xff}, \
            "a finite code point is not produced"
        assert seen & {0x7f, 0xff}, "no NaN is produced"


_both("paged_fp8_kv_write", _check_write,
      [(64, False), (64, True), (128, False), (128, True)])


# ---------------------------------------------------------------------------
# 2. paged_attention_decode over fp8 pools
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _decode_case(hd, Hq, Hkv, ps, seq_lens):
    """The bf16 file's case (q, table, lens) with fp8 pools quantised from
    its K/V; float64 reference over the dequantised pools and that file's
    error term (2*(s_max + 4) + L) * 2**-23 * max|v|, see tpa._case."""
    c = tpa._case(hd, Hq, Hkv, ps, seq_lens)
    f = _fp8_pools(c, Hkv, 11 + hd + Hq + Hkv + ps)
    B, g = len(seq_lens), Hq // Hkv
    ref = torch.zeros(B, Hq, hd, dtype=F64)
    extra = torch.zeros(B, Hq, 1, dtype=F64)
    for b, n in enumerate(seq_lens):
        if n == 0:
            continue
        k = tpp._gather(f["kd"], c["table"], b, n, ps)   # [Hkv, n, hd]
        v = tpp._gather(f["vd"], c["table"], b, n, ps)
        s = torch.matmul(_f64(c["q"][b]).view(Hkv, g, hd),
                         k.transpose(1, 2)) * c["scale"]
        ref[b] = torch.matmul(torch.softmax(s, -1), v).view(Hq, hd)
        s_max = s.abs().amax(-1).view(Hq)
        v_max = v.abs().amax((1, 2)).repeat_interleave(g)
        extra[b, :, 0] = (2 * (s_max + 4) + n) * 2.0 ** -23 * v_max
    return dict(c, ref=ref, extra=extra, **f)


def _decode(device, c, ns, kq=None, vq=None):
    kq = c["kq"] if kq is None else kq
    vq = c["vq"] if vq is None else vq
    return ops.paged_attention_decode(
        c["q"].to(device), kq.to(device), vq.to(device),
        c["table"].to(device), c["lens"].to(device), num_splits=ns,
        k_scale=c["ks"].to(device), v_scale=c["vs"].to(device))


def _check_decode_ragged(device, hd, Hq, Hkv, ps):
    c = _decode_case(hd, Hq, Hkv, ps, tpa._ragged_lens(ps))
    for ns in (0, 1):
        out = _decode(device, c, ns)
        name = f"fp8_ragged_{device}_hd{hd}_q{Hq}_kv{Hkv}_ps{ps}_ns{ns}"
        assert out.dtype == BF16 and out.shape == c["q"].shape
        tpa._report(name, out, c)
        assert bool(out.isfinite().all()), name
        assert int(_bits(out[4]).count_nonzero()) == 0, \
            f"{name}: inactive row is not exactly zero"
        tpa.assert_bf16_ulp(out, c["ref"], c["extra"], msg=name)


_both("paged_fp8_decode_ragged", _check_decode_ragged, CASES)


def _check_decode_long_splits(device, hd, Hq, Hkv, ps):
    c = _decode_case(hd, Hq, Hkv, ps, tuple(tpa.LONG_LENS))
    outs = {}
    for ns in (1, 2, 4, 7):
        out = _decode(device, c, ns)
        name = f"fp8_long_{device}_hd{hd}_q{Hq}_kv{Hkv}_ps{ps}_ns{ns}"
        tpa._report(name, out, c)
        tpa.assert_bf16_ulp(out, c["ref"], c["extra"], msg=name)
        outs[ns] = _f64(out).cpu()
    twice = 2 * (2.0 ** -7 * c["ref"].abs() + c["extra"])
    assert bool(((outs[1] - outs[4]).abs() <= twice).all()), \
        "num_splits 1 and 4 disagree"


_both("paged_fp8_decode_long_splits", _check_decode_long_splits, CASES)


def _check_decode_poison(device, hd, Hq, Hkv, ps, lens, ns):
    """Dead positions holding the NaN byte 0x7f or 0x7e (= 448) change
    nothing: they are never loaded."""
    c = _decode_case(hd, Hq, Hkv, ps, lens)
    clean = _decode(device, c, ns, _poison(c["kq"], c["valid"], 0),
                    _poison(c["vq"], c["valid"], 0))
    tpa.assert_bf16_ulp(clean, c["ref"], c["extra"], msg="zeroed baseline")
    for byte in (0x7f, 0x7e):
        kq = _poison(c["kq"], c["valid"], byte)
        vq = _poison(c["vq"], c["valid"], byte)
        assert int((kq.view(torch.uint8) == byte).sum()) > 0
        out = _decode(device, c, ns, kq, vq)
        assert torch.equal(_bits(out), _bits(clean)), \
            f"poison {byte:#x} reached the output (ns={ns})"


_both("paged_fp8_decode_poison", _check_decode_poison,
      [(hd, Hq, Hkv, ps, tpa._ragged_lens(ps), 1)
       for hd, Hq, Hkv, ps in CASES]
      + [(128, 8, 2, 16, tuple(tpa.LONG_LENS), 4),
         (64, 8, 1, 64, tuple(tpa.LONG_LENS), 7)])


# ---------------------------------------------------------------------------
# 3. paged_attention_prefill over fp8 pools
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _prefill_case(hd, Hq, Hkv, ps, rows):
    """The bf16 file's case with fp8 pools; reference and both error terms
    from that file's _reference over the dequantised pools."""
    c = tpp._case(hd, Hq, Hkv, ps, rows)
    f = _fp8_pools(c, Hkv, 23 + hd + Hq + Hkv + ps)
    ref, e32, eP = tpp._reference(c["q"], f["kd"], f["vd"], c["table"], rows,
                                  c["scale"])
    return dict(c, ref=ref, e32=e32, eP=eP, **f)


def _prefill(device, c, kq=None, vq=None, lens=None):
    Hq, hd = c["q"].shape[1:]
    wide = c["wide"].to(device)
    q = wide[:, :Hq * hd].view(-1, Hq, hd)
    kq = c["kq"] if kq is None else kq
    vq = c["vq"] if vq is None else vq
    lens = c["lens"] if lens is None else lens
    return ops.paged_attention_prefill(
        q, kq.to(device), vq.to(device), c["table"].to(device),
        c["cu"].to(device), lens.to(device), c["max_q"],
        k_scale=c["ks"].to(device), v_scale=c["vs"].to(device))


def _check_prefill_ragged(device, hd, Hq, Hkv, ps):
    """ctx = 0, ctx > 0, qlen = 1, qlen = 0, a key-tile boundary at 64 keys,
    a query-tile boundary at 128/G tokens (the 130-token row); then a row
    with qlen > seq_lens, which must come back zero."""
    c = _prefill_case(hd, Hq, Hkv, ps, tpp._ragged_rows(ps))
    out = _prefill(device, c)
    name = f"fp8_prefill_ragged_{device}_hd{hd}_q{Hq}_kv{Hkv}_ps{ps}"
    assert out.dtype == BF16 and out.shape == c["q"].shape
    extra = tpp._extra(device, c)
    tpp._report(name, out, c, extra)
    assert bool(out.isfinite().all()), name
    tpp.assert_bf16_ulp(out, c["ref"], extra, msg=name)
    lens = c["lens"].clone()
    lens[3] = 1                      # row 3: qlen 2 > seq_len 1
    t0 = int(c["cu"][3])
    bad = _prefill(device, c, lens=lens)
    assert int(_bits(bad[t0:t0 + 2]).count_nonzero()) == 0
    assert torch.equal(_bits(bad[:t0]), _bits(out[:t0]))
    assert torch.equal(_bits(bad[t0 + 2:]), _bits(out[t0 + 2:]))


_both("paged_fp8_prefill_ragged", _check_prefill_ragged, CASES)


def _check_prefill_poison(device, hd, Hq, Hkv, ps):
    c = _prefill_case(hd, Hq, Hkv, ps, tpp._ragged_rows(ps))
    clean = _prefill(device, c, _poison(c["kq"], c["valid"], 0),
                     _poison(c["vq"], c["valid"], 0))
    tpp.assert_bf16_ulp(clean, c["ref"], tpp._extra(device, c),
                        msg="zeroed baseline")
    for byte in (0x7f, 0x7e):
        out = _prefill(device, c, _poison(c["kq"], c["valid"], byte),
                       _poison(c["vq"], c["valid"], byte))
        assert torch.equal(_bits(out), _bits(clean)), \
            f"poison {byte:#x} reached the output"


_both("paged_fp8_prefill_poison", _check_prefill_poison, CASES)


# ---------------------------------------------------------------------------
# 4. prefill with qlen = 1 rows against decode, same fp8 pools
# ---------------------------------------------------------------------------
def _check_consistency(device, hd, Hq, Hkv, ps):
    """Within the sum of the two ops' bounds: decode's (no P rounding) and
    prefill's (with it on the GPU)."""
    rows = ((0, 1), (ps - 1, 1), (ps, 1), (3 * 64 + 5, 1), (599, 1))
    c = _prefill_case(hd, Hq, Hkv, ps, rows)
    pre = _prefill(device, c)
    extra = tpp._extra(device, c)
    tpp.assert_bf16_ulp(pre, c["ref"], extra, msg="prefill qlen=1")
    dec = ops.paged_attention_decode(
        c["q"].contiguous().to(device), c["kq"].to(device),
        c["vq"].to(device), c["table"].to(device), c["lens"].to(device),
        num_splits=1, k_scale=c["ks"].to(device), v_scale=c["vs"].to(device))
    tpa.assert_bf16_ulp(dec, c["ref"], c["e32"], msg="decode")
    diff = (_f64(pre) - _f64(dec)).abs().cpu()
    bound = 2 * 2.0 ** -7 * c["ref"].abs() + extra + c["e32"]
    _note(f"fp8_prefill_vs_decode_{device}_hd{hd}_q{Hq}_kv{Hkv}_ps{ps}",
          (diff / (bound + 1e-30)).max().item())
    assert bool((diff <= bound).all()), "prefill and decode disagree"


_both("paged_fp8_prefill_decode_consistency", _check_consistency, CASES)


# ---------------------------------------------------------------------------
# 5. argument errors
# ---------------------------------------------------------------------------
def _check_arguments(device):
    Hq, Hkv, ps, hd = 4, 2, 16, 64
    z = lambda dt: torch.zeros(4, Hkv, ps, hd, device=device).to(dt)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device=device)
    ones = torch.ones(Hkv, device=device)
    q2 = torch.zeros(2, Hq, hd, dtype=BF16, device=device)
    q3 = torch.zeros(3, Hq, hd, dtype=BF16, device=device)
    kn = torch.zeros(3, Hkv, hd, dtype=BF16, device=device)
    table = torch.zeros(2, 3, dtype=torch.int32, device=device)

    def write(kp, vp, ks=None, vs=None):
        ops.paged_kv_write(kn, kn, kp, vp, i32(0, 1, 2), ks, vs)

    def decode(kp, vp, ks=None, vs=None):
        return ops.paged_attention_decode(q2, kp, vp, table, i32(1, 1),
                                          num_splits=1, k_scale=ks, v_scale=vs)

    def prefill(kp, vp, ks=None, vs=None):
        return ops.paged_attention_prefill(q3, kp, vp, table, i32(0, 1, 3),
                                           i32(1, 2), 2, k_scale=ks,
                                           v_scale=vs)

    # the supported forms of the same calls
    write(z(FP8), z(FP8))
    write(z(FP8), z(FP8), ones, ones * 0.5)
    assert decode(z(FP8), z(FP8)).shape == (2, Hq, hd)
    assert decode(z(FP8), z(FP8), ones, ones).dtype == BF16
    assert prefill(z(FP8), z(FP8), ones, None).shape == (3, Hq, hd)
    bad_scales = [torch.ones(Hkv + 1, device=device),
                  torch.ones(Hkv, 1, device=device),
                  torch.ones(Hkv, device=device, dtype=torch.float64),
                  torch.ones(Hkv, device=device, dtype=BF16)]
    if device == "cpu":  # values are looked at only where that is no sync
        bad_scales += [torch.tensor([1.0, 0.0]), torch.tensor([1.0, -2.0]),
                       torch.tensor([float("inf"), 1.0]),
                       torch.tensor([float("nan"), 1.0])]
    others = [torch.float8_e5m2]
    for n in ("float8_e4m3fnuz", "float8_e5m2fnuz"):
        if hasattr(torch, n):
            others.append(getattr(torch, n))
    for op in (write, decode, prefill):
        with pytest.raises(RAISES):      # mixed pool dtypes
            op(z(FP8), z(BF16))
        with pytest.raises(RAISES):
            op(z(BF16), z(FP8))
        for dt in others:                # e5m2 and the fnuz encodings
            with pytest.raises(RAISES):
                op(z(dt), z(dt))
        with pytest.raises(ValueError):  # scales with bf16 pools
            op(z(BF16), z(BF16), ones, ones)
        with pytest.raises(ValueError):
            op(z(BF16), z(BF16), None, ones)
        for s in bad_scales:
            with pytest.raises(RAISES):
                op(z(FP8), z(FP8), s, ones)
            with pytest.raises(RAISES):
                op(z(FP8), z(FP8), ones, s)
    # the unquantised errors stay errors with fp8 pools
    with pytest.raises(RAISES):
        ops.paged_attention_decode(q2.to(torch.float16), z(FP8), z(FP8),
                                   table, i32(1, 1), num_splits=1)
    with pytest.raises(RAISES):          # page_size 8
        p8 = torch.zeros(4, Hkv, 8, hd, device=device).to(FP8)
        decode(p8, p8.clone())
    with pytest.raises(RAISES):          # head_dim 96
        p96 = torch.zeros(4, Hkv, ps, 96, device=device).to(FP8)
        ops.paged_attention_decode(
            torch.zeros(2, Hq, 96, dtype=BF16, device=device), p96,
            p96.clone(), table, i32(1, 1), num_splits=1)
    with pytest.raises(RAISES):          # group 3
        ops.paged_attention_decode(
            torch.zeros(2, 6, hd, dtype=BF16, device=device), z(FP8), z(FP8),
            table, i32(1, 1), num_splits=1)
    with pytest.raises(RAISES):          # non-contiguous pool
        wide = torch.zeros(4, Hkv, 32, hd, device=device).to(FP8)
        decode(wide[:, :, :16], wide[:, :, :16])


_both("paged_fp8_arguments", _check_arguments)


# ---------------------------------------------------------------------------
# 6. Engine, CPU: exact tokens against a fake-quantised unquantised engine
# ---------------------------------------------------------------------------
def _cpu_model(seed=31):
    torch.manual_seed(seed)
    return Llama(llama_tiny()).eval()


def _cpu_prompts(cfg):
    gen = torch.Generator().manual_seed(3)
    p = [torch.randint(0, cfg.vocab_size, (n,), generator=gen).tolist()
         for n in (17, 5, 29, 11)]
    p[2] = p[0][:16] + p[2][16:]    # shares a full page with the first
    return p


def _run_engine(model, prompts, new=12, **kw):
    eng = BatchedGenerator(model, max_batch=2, max_len=64, kv="paged",
                           page_size=16, **kw)
    rids = [eng.submit(p, max_new_tokens=new) for p in prompts]
    out = eng.run()
    assert eng._pkv.free_pages == eng._pkv.num_pages
    return eng, [out[r] for r in rids]


@pytest.mark.parametrize("calibrated", [False, True],
                         ids=["unit-scales", "calibrated"])
@pytest.mark.parametrize("kw", [
    dict(prefill="cache"), dict(prefill="paged"),
    dict(prefill="cache", prefill_chunk=4),
    dict(prefill="paged", prefill_chunk=4), dict(prefix_cache=True)],
    ids=["cache", "paged", "cache-chunk4", "paged-chunk4", "prefix"])
def test_fp8_engine_matches_fake_quantised_engine_cpu(monkeypatch, kw,
                                                      calibrated):
    """The fp8 engine against the unquantised engine whose paged_kv_write
    round-trips k_new / v_new through the contract's quantise-dequantise:
    both then read the same fp32 values through the same reference code, so
    the greedy tokens are equal. (Equality with the plain engine is not
    required: quantisation changes tokens.)"""
    model = _cpu_model()
    prompts = _cpu_prompts(model.cfg)
    scales = calibrate_kv_scales(model, prompts[2]) if calibrated else None
    eng, got = _run_engine(model, prompts, kv_dtype="fp8", kv_scales=scales,
                           **kw)
    assert eng._pkv.k[0].dtype == FP8
    if kw.get("prefix_cache"):
        assert eng.prefix_stats["hit_tokens"] == 16

    n_layers, n_kv = model.cfg.n_layers, model.cfg.n_kv_heads
    ks, vs = scales if calibrated else (torch.ones(n_layers, n_kv),) * 2
    real_write = ops.paged_kv_write
    state = {}

    def fake_quant_write(k_new, v_new, k_pages, v_pages, slot_map,
                         k_scale=None, v_scale=None):
        assert k_scale is None and v_scale is None
        i = [j for j, p in enumerate(state["eng"]._pkv.k) if p is k_pages][0]
        s_k, s_v = ks[i].view(1, n_kv, 1), vs[i].view(1, n_kv, 1)
        real_write(_quant(k_new, s_k).float() * s_k,
                   _quant(v_new, s_v).float() * s_v, k_pages, v_pages,
                   slot_map)

    monkeypatch.setattr(ops, "paged_kv_write", fake_quant_write)
    eng2 = BatchedGenerator(model, max_batch=2, max_len=64, kv="paged",
                            page_size=16, **kw)
    state["eng"] = eng2
    rids = [eng2.submit(p, max_new_tokens=12) for p in prompts]
    out = eng2.run()
    assert eng2._pkv.k[0].dtype == torch.float32
    assert got == [out[r] for r in rids]
    for p, toks in zip(prompts, got):
        assert toks[:len(p)] == p and len(toks) == len(p) + 12


def test_fp8_engine_arguments():
    model = _cpu_model()
    with pytest.raises(ValueError, match="paged"):
        BatchedGenerator(model, max_batch=2, max_len=64, kv_dtype="fp8")
    with pytest.raises(ValueError, match="kv_dtype"):
        BatchedGenerator(model, max_batch=2, max_len=64, kv="paged",
                         kv_dtype="e5m2")
    with pytest.raises(ValueError, match="kv_dtype"):
        BatchedGenerator(model, max_batch=2, max_len=64, kv="paged",
                         kv_dtype="bf16")
    n_layers, n_kv = model.cfg.n_layers, model.cfg.n_kv_heads
    ones = torch.ones(n_layers, n_kv)
    with pytest.raises(ValueError):      # scales without fp8
        BatchedGenerator(model, max_batch=2, max_len=64, kv="paged",
                         kv_scales=(ones, ones))
    for bad in (torch.ones(n_layers, n_kv + 1), torch.zeros(n_layers, n_kv),
                -ones, ones * float("inf"), torch.ones(n_kv)):
        with pytest.raises(ValueError):
            BatchedGenerator(model, max_batch=2, max_len=64, kv="paged",
                             kv_dtype="fp8", kv_scales=(ones, bad))
        with pytest.raises(ValueError):
            PagedKVCache(model.cfg, 4, 16, 2, 4, torch.device("cpu"),
                         torch.float32, kv_dtype="fp8", k_scales=bad)


# ---------------------------------------------------------------------------
# 7. calibrate_kv_scales
# ---------------------------------------------------------------------------
def test_calibrate_kv_scales_cpu(monkeypatch):
    model = _cpu_model(47)
    cfg = model.cfg
    prompt = _cpu_prompts(cfg)[2]
    ks, vs = calibrate_kv_scales(model, prompt)
    for s in (ks, vs):
        assert s.shape == (cfg.n_layers, cfg.n_kv_heads)
        assert s.dtype == torch.float32 and s.device.type == "cpu"
        assert bool(((s > 0) & s.isfinite()).all())
    k2, v2 = calibrate_kv_scales(model, torch.tensor([prompt]), margin=2.0)
    assert torch.allclose(k2, 2 * ks) and torch.allclose(v2, 2 * vs)

    # what the engine writes for that prompt: spy on paged_kv_write
    real_write = ops.paged_kv_write
    seen = {}

    def spy(k_new, v_new, k_pages, v_pages, slot_map, k_scale=None,
            v_scale=None):
        i = [j for j, p in enumerate(eng._pkv.k) if p is k_pages][0]
        if i not in seen:   # the prefill call of each layer
            seen[i] = (k_new.clone(), v_new.clone(), slot_map.clone())
        real_write(k_new, v_new, k_pages, v_pages, slot_map, k_scale, v_scale)

    monkeypatch.setattr(ops, "paged_kv_write", spy)
    # The unquantised engine's prefill writes what the calibration walk
    # saw, up to fp32 rounding of a different attention implementation:
    # scale * 448 covers every head's amax, and with margin 1.0 equals it.
    eng = BatchedGenerator(model, max_batch=1, max_len=64, kv="paged",
                           prefill="paged")
    eng.submit(prompt, max_new_tokens=2)
    eng.step()
    assert sorted(seen) == list(range(cfg.n_layers))
    tol = 1e-4
    for i, (k_new, v_new, _) in seen.items():
        assert k_new.shape[0] == len(prompt)
        for x, s in ((k_new, ks[i]), (v_new, vs[i])):
            amax = x.float().abs().amax((0, 2))
            assert bool((s * 448 >= amax * (1 - tol)).all())
            assert bool((s * 448 <= amax * (1 + tol)).all())

    # An engine built with the result runs. In layer 0, whose k/v do not
    # depend on quantised attention, nothing is clamped; in every layer the
    # 448 code is written only for what rounds there (|x|/scale >= 432).
    seen.clear()
    eng = BatchedGenerator(model, max_batch=1, max_len=64, kv="paged",
                           prefill="paged", kv_dtype="fp8",
                           kv_scales=(ks, vs))
    rid = eng.submit(prompt, max_new_tokens=2)
    eng.step()
    assert sorted(seen) == list(range(cfg.n_layers))
    for i, (k_new, v_new, sm) in seen.items():
        for x, s, pool in ((k_new, ks[i], eng._pkv.k[i]),
                           (v_new, vs[i], eng._pkv.v[i])):
            y = (x.float() / s.view(1, -1, 1)).abs()
            if i == 0:
                assert bool((y <= 448 * (1 + 1e-6)).all()), "clamped"
                assert bool((y.amax((0, 2)) >= 448 * (1 - 1e-6)).all())
            ps = pool.shape[2]
            page, off = (sm // ps).long(), (sm % ps).long()
            code = pool[page, :, off].view(torch.uint8) & 0x7f
            assert bool((y[code == 0x7e] >= 432 * (1 - 1e-6)).all())
            assert int((code == 0x7f).sum()) == 0
    out = eng.run()
    assert len(out[rid]) == len(prompt) + 2


# ---------------------------------------------------------------------------
# 9. memory
# ---------------------------------------------------------------------------
def test_fp8_cache_is_one_byte_per_element():
    cfg = llama_tiny()
    dev = torch.device("cpu")
    a = PagedKVCache(cfg, 6, 16, 2, 3, dev, torch.bfloat16)
    b = PagedKVCache(cfg, 6, 16, 2, 3, dev, torch.bfloat16, kv_dtype="fp8")
    assert a.kv_dtype is None and a.k_scale == [None] * cfg.n_layers
    for i in range(cfg.n_layers):
        for p, r in ((b.k[i], a.k[i]), (b.v[i], a.v[i])):
            assert p.dtype == FP8 and p.element_size() == 1
            assert p.shape == r.shape and r.element_size() == 2
        for s in (b.k_scale[i], b.v_scale[i]):
            assert s.dtype == torch.float32
            assert s.shape == (cfg.n_kv_heads,) and bool((s == 1).all())
    eng = BatchedGenerator(_cpu_model(), max_batch=3, max_len=40, kv="paged",
                           kv_dtype="fp8")
    assert eng._pkv.num_pages == 3 * 3    # the default keeps token capacity


# ---------------------------------------------------------------------------
# 8. Engine, GPU (bf16 model)
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_model():
    cfg = llama_tiny(max_seq_len=192)
    torch.manual_seed(11)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with torch.device("cuda"):
            model = Llama(cfg).eval()
    finally:
        torch.set_default_dtype(prev)
    return model


@pytest.fixture(scope="module")
def gpu_scales(gpu_model):
    prompts = tpe._gpu_prompts(gpu_model.cfg)
    ks, vs = calibrate_kv_scales(gpu_model, prompts[2], margin=1.5)
    cfg = gpu_model.cfg
    assert ks.shape == vs.shape == (cfg.n_layers, cfg.n_kv_heads)
    assert ks.dtype == torch.float32
    return ks, vs


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_fp8_decode_graph_matches_eager_gpu(gpu_model, gpu_scales):
    """(a) graph and eager give identical tokens with one captured graph;
    (c) every emitted token passes the teacher-forced check (a gross check:
    wrong scales or garbage reads, not rounding)."""
    model = gpu_model
    prompts = tpe._gpu_prompts(model.cfg)

    def run(graph):
        eng = BatchedGenerator(model, max_batch=3, max_len=96, graph=graph,
                               kv="paged", page_size=16, kv_dtype="fp8",
                               kv_scales=gpu_scales)
        assert eng._pkv.k[0].dtype == FP8
        rids = [eng.submit(p, max_new_tokens=12) for p in prompts[:2]]
        for _ in range(3):  # staggered join
            eng.step()
        rids += [eng.submit(p, max_new_tokens=12) for p in prompts[2:]]
        out = eng.run()
        assert eng._pkv.free_pages == eng._pkv.num_pages
        return eng, [out[r] for r in rids]

    _, eager = run(False)
    eng, graphed = run(True)
    assert eager == graphed
    assert eng._use_graph and len(eng._graphs) == 1
    for p, toks in zip(prompts, graphed):
        assert len(toks) == len(p) + 12
        tpe._assert_teacher_forced(model, len(p), toks)


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("prefill", ["cache", "paged"])
@pytest.mark.parametrize("calibrated", [False, True],
                         ids=["unit-scales", "calibrated"])
def test_fp8_engine_layer0_pages_are_quantised_bf16_pages_gpu(
        gpu_model, gpu_scales, prefill, calibrated):
    """(b) Layer 0's K/V do not depend on attention output, so after the
    same admissions the fp8 engine's layer-0 pages are, byte for byte, the
    contract's quantisation of the bf16 engine's, at the prompts'
    positions and at the first decoded token's."""
    model = gpu_model
    prompts = tpe._gpu_prompts(model.cfg)
    scales = gpu_scales if calibrated else None
    kw = dict(max_batch=4, max_len=96, graph=False, kv="paged", page_size=16,
              prefill=prefill)
    ref_eng = BatchedGenerator(model, **kw)
    eng = BatchedGenerator(model, kv_dtype="fp8", kv_scales=scales, **kw)
    for e in (ref_eng, eng):
        for p in prompts:
            e.submit(p, max_new_tokens=4)
        e.step()
    n_kv = model.cfg.n_kv_heads
    ones = torch.ones(n_kv)
    ks = gpu_scales[0][0] if calibrated else ones
    vs = gpu_scales[1][0] if calibrated else ones
    checked = 0
    for slot, p in enumerate(prompts):
        assert eng._pkv.pages_of(slot) == ref_eng._pkv.pages_of(slot)
        # the prompt, and the first new token (written by the decode step);
        # its token may differ between the engines, so only the prompt's
        # positions are compared
        sm = torch.tensor(eng._pkv.token_slots(slot, 0, len(p)))
        page, off = sm // 16, sm % 16
        for pool, ref_pool, s in ((eng._pkv.k[0], ref_eng._pkv.k[0], ks),
                                  (eng._pkv.v[0], ref_eng._pkv.v[0], vs)):
            got = pool.cpu()[page, :, off].view(torch.uint8)
            want = _quant(ref_pool.cpu()[page, :, off],
                          s.view(1, n_kv, 1)).view(torch.uint8)
            assert torch.equal(got, want), (slot, prefill)
            checked += got.numel()
    assert checked == 2 * sum(len(p) for p in prompts) * n_kv * 64
    eng.run()
    ref_eng.run()
    assert eng._pkv.free_pages == eng._pkv.num_pages


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_fp8_prefix_cache_gpu(gpu_model, gpu_scales):
    """(d) Two requests sharing a 32-token prefix, admitted in different
    steps: the second is served from the first's fp8 pages."""
    model = gpu_model
    gen = torch.Generator().manual_seed(5)
    rnd = lambda n: torch.randint(0, model.cfg.vocab_size, (n,),
                                  generator=gen).tolist()
    shared = rnd(32)
    prompts = [shared + rnd(7), shared + rnd(12)]
    eng = BatchedGenerator(model, max_batch=2, max_len=96, kv="paged",
                           page_size=16, prefix_cache=True, kv_dtype="fp8",
                           kv_scales=gpu_scales)
    r0 = eng.submit(prompts[0], max_new_tokens=8)
    eng.step()
    eng.step()
    r1 = eng.submit(prompts[1], max_new_tokens=8)
    out = eng.run()
    assert eng.prefix_stats["hit_tokens"] == 32
    assert eng.cached_tokens[r1] == 32 and eng.cached_tokens[r0] == 0
    for rid, p in ((r0, prompts[0]), (r1, prompts[1])):
        assert len(out[rid]) == len(p) + 8
        tpe._assert_teacher_forced(model, len(p), out[rid])
    assert eng._pkv.free_pages == eng._pkv.num_pages
