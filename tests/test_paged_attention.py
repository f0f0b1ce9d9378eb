"""Paged KV cache ops: ops.paged_kv_write and ops.paged_attention_decode.

Same scheme as tests/test_ops_edges.py: every kernel case is a
`_check(device, ...)` run on "cpu" against the project's fp32 reference
path (this proves the test and its tolerance on any machine) and on "cuda"
under the gpu marker, where it runs the gfx950 kernels. Attention results
are compared with a float64 reference built from the same bf16 inputs under
the one-bf16-ulp rule (assert_bf16_ulp, copied from test_ops_edges.py).

Lines starting with "[edges]" report measured errors; run with -s.
"""
import functools

import pytest
import torch

from kubetorch_amd import ops

BF16 = torch.bfloat16
F64 = torch.float64

# (hd, Hq, Hkv): groups 2 (llama_tiny), 4 (8B), 1 (MHA), 8 (70B)
CONFIGS = [(64, 4, 2), (128, 8, 2), (128, 8, 8), (128, 8, 1)]
PAGE_SIZES = [16, 64]
CASES = [c + (ps,) for c in CONFIGS for ps in PAGE_SIZES]
LONG_LENS = [3 * 64 + 5, 600, 17]
RAISES = (RuntimeError, ValueError)


def _f64(t):
    return t.detach().to(F64)


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


# ---------------------------------------------------------------------------
# Case construction (CPU tensors, built once per case and never modified)
# ---------------------------------------------------------------------------
def _pages_for(n, ps):
    return -(-n // ps)


def _block_table(seq_lens, ps, gen):
    """Physical pages from a seeded permutation of a pool larger than
    needed, dealt out round-robin so the sequences' pages interleave.
    max_blocks exceeds every row's use; unused entries are -1."""
    need = [_pages_for(n, ps) for n in seq_lens]
    num_pages = 2 * sum(need) + 5
    max_blocks = max(need) + 3
    perm = torch.randperm(num_pages, generator=gen).tolist()
    table = torch.full((len(seq_lens), max_blocks), -1, dtype=torch.int32)
    nxt = 0
    for blk in range(max(need)):
        for b, n in enumerate(need):
            if blk < n:
                table[b, blk] = perm[nxt]
                nxt += 1
    return table, num_pages


def _valid_mask(table, seq_lens, num_pages, ps):
    """[num_pages, ps] bool: positions that hold a valid token."""
    valid = torch.zeros(num_pages, ps, dtype=torch.bool)
    for b, n in enumerate(seq_lens):
        for t in range(n):
            valid[int(table[b, t // ps]), t % ps] = True
    return valid


@functools.lru_cache(maxsize=None)
def _case(hd, Hq, Hkv, ps, seq_lens, seed=0):
    """Inputs plus the float64 reference and its fp32 error term.

    extra_abs per output row = (2*(s_max + 4) + L) * 2**-23 * max|v|:
    the exp argument (a scaled score of size <= s_max, computed in fp32
    and shifted by the running max) carries an absolute error of about
    (s_max + 4) * 2**-23 in the kernel and as much in its exp, which is a
    relative error of the probabilities; the L-term fp32 sums of p and of
    p*v add L * 2**-23. The output is a convex combination of the row's v,
    so every term scales with max|v| over the row's valid tokens.
    """
    gen = torch.Generator().manual_seed(1000 * seed + 7 * hd + Hq + Hkv + ps)
    B = len(seq_lens)
    table, num_pages = _block_table(seq_lens, ps, gen)
    shape = (num_pages, Hkv, ps, hd)
    q = (torch.randn(B, Hq, hd, generator=gen) * 1.5).to(BF16)
    kp = torch.randn(shape, generator=gen).to(BF16)
    vp = torch.randn(shape, generator=gen).to(BF16)
    lens = torch.tensor(seq_lens, dtype=torch.int32)
    scale = hd ** -0.5
    g = Hq // Hkv
    ref = torch.zeros(B, Hq, hd, dtype=F64)
    extra = torch.zeros(B, Hq, 1, dtype=F64)
    for b, n in enumerate(seq_lens):
        if n == 0:
            continue
        page = torch.tensor([int(table[b, t // ps]) for t in range(n)])
        off = torch.tensor([t % ps for t in range(n)])
        k = _f64(kp[page, :, off]).transpose(0, 1)  # [Hkv, n, hd]
        v = _f64(vp[page, :, off]).transpose(0, 1)
        s = torch.matmul(_f64(q[b]).view(Hkv, g, hd), k.transpose(1, 2)) * scale
        ref[b] = torch.matmul(torch.softmax(s, -1), v).view(Hq, hd)
        s_max = s.abs().amax(-1).view(Hq)
        v_max = v.abs().amax((1, 2)).repeat_interleave(g)
        extra[b, :, 0] = (2 * (s_max + 4) + n) * 2.0 ** -23 * v_max
    valid = _valid_mask(table, seq_lens, num_pages, ps)
    return dict(q=q, kp=kp, vp=vp, table=table, lens=lens, ref=ref,
                extra=extra, valid=valid, scale=scale)


def _run(device, c, num_splits, kp=None, vp=None):
    kp = c["kp"] if kp is None else kp
    vp = c["vp"] if vp is None else vp
    return ops.paged_attention_decode(
        c["q"].to(device), kp.to(device), vp.to(device),
        c["table"].to(device), c["lens"].to(device), num_splits=num_splits)


def _report(name, out, c):
    err = (_f64(out).cpu() - c["ref"]).abs()
    bound = 2.0 ** -7 * c["ref"].abs() + c["extra"] + 1e-30
    _note(name + "_max_abs_err", err.max().item())
    _note(name + "_max_err_over_bound", (err / bound).max().item())


# ---------------------------------------------------------------------------
# paged_attention_decode
# ---------------------------------------------------------------------------
def _ragged_lens(ps):
    # single token, page tail, exact page, page crossing, inactive row
    return (1, ps - 1, ps, ps + 1, 0)


def _check_ragged(device, hd, Hq, Hkv, ps):
    c = _case(hd, Hq, Hkv, ps, _ragged_lens(ps))
    for ns in (0, 1):
        out = _run(device, c, ns)
        name = f"paged_ragged_{device}_hd{hd}_q{Hq}_kv{Hkv}_ps{ps}_ns{ns}"
        assert out.dtype == BF16 and out.shape == c["q"].shape
        _report(name, out, c)
        assert bool(out.isfinite().all()), name
        assert int(_bits(out[4]).count_nonzero()) == 0, \
            f"{name}: inactive row is not exactly zero"
        assert_bf16_ulp(out, c["ref"], c["extra"], msg=name)


_both("paged_attention_ragged", _check_ragged, CASES)


def _check_long_splits(device, hd, Hq, Hkv, ps):
    """Several pages per split and a partial last page; 7 splits leave
    empty splits for the short rows and uneven ranges for the long ones."""
    c = _case(hd, Hq, Hkv, ps, tuple(LONG_LENS))
    outs = {}
    for ns in (1, 2, 4, 7):
        out = _run(device, c, ns)
        name = f"paged_long_{device}_hd{hd}_q{Hq}_kv{Hkv}_ps{ps}_ns{ns}"
        _report(name, out, c)
        assert_bf16_ulp(out, c["ref"], c["extra"], msg=name)
        outs[ns] = _f64(out).cpu()
    twice = 2 * (2.0 ** -7 * c["ref"].abs() + c["extra"])
    diff = (outs[1] - outs[4]).abs()
    _note(f"paged_long_{device}_hd{hd}_q{Hq}_kv{Hkv}_ps{ps}_ns1_vs_ns4",
          diff.max().item())
    assert bool((diff <= twice).all()), "num_splits 1 and 4 disagree"


_both("paged_attention_long_splits", _check_long_splits, CASES)


def _poisoned(c, value):
    """K and V with `value` at every position that holds no valid token:
    all of every page the table does not reference, and positions >=
    seq_len of each last page."""
    dead = ~c["valid"][:, None, :, None]
    fill = torch.tensor(value, dtype=BF16)
    return (torch.where(dead, fill, c["kp"]), torch.where(dead, fill, c["vp"]))


def _check_poison(device, hd, Hq, Hkv, ps, lens, ns):
    c = _case(hd, Hq, Hkv, ps, lens)
    clean = _run(device, c, ns, *_poisoned(c, 0.0))
    assert_bf16_ulp(clean, c["ref"], c["extra"], msg="zeroed baseline")
    for value in (float("nan"), float("inf")):
        kp, vp = _poisoned(c, value)
        assert not bool(kp.isfinite().all())
        out = _run(device, c, ns, kp, vp)
        assert torch.equal(_bits(out), _bits(clean)), \
            f"poison {value} reached the output (ns={ns})"


_both("paged_attention_poison", _check_poison,
      [(hd, Hq, Hkv, ps, _ragged_lens(ps), 1) for hd, Hq, Hkv, ps in CASES]
      + [(128, 8, 2, 16, tuple(LONG_LENS), 4),
         (64, 4, 2, 64, tuple(LONG_LENS), 7)])


def _check_deterministic(device):
    c = _case(128, 8, 2, 16, tuple(LONG_LENS))
    for ns in (1, 4):
        a, b = _run(device, c, ns), _run(device, c, ns)
        assert torch.equal(_bits(a), _bits(b)), f"ns={ns} not deterministic"


_both("paged_attention_deterministic", _check_deterministic)


def _check_arguments(device):
    """Unsupported configurations raise; on the GPU these stop at the
    host-side checks, nothing is launched."""
    def call(hd=64, Hq=4, Hkv=2, ps=16, qdtype=BF16, pool=None):
        q = torch.zeros(2, Hq, hd, dtype=qdtype, device=device)
        if pool is None:
            pool = torch.zeros(4, Hkv, ps, hd, dtype=BF16, device=device)
        table = torch.zeros(2, 3, dtype=torch.int32, device=device)
        lens = torch.ones(2, dtype=torch.int32, device=device)
        return ops.paged_attention_decode(q, pool, pool.clone() if
                                          pool.is_contiguous() else pool,
                                          table, lens, num_splits=1)

    assert call().shape == (2, 4, 64)  # the supported form of the same call
    with pytest.raises(RAISES):
        call(qdtype=torch.float16)
    with pytest.raises(RAISES):
        call(hd=96)
    with pytest.raises(RAISES):
        call(ps=8)
    with pytest.raises(RAISES):
        call(Hq=6, Hkv=2)
    wide = torch.zeros(4, 2, 32, 64, dtype=BF16, device=device)
    with pytest.raises(RAISES):
        call(pool=wide[:, :, :16])
    q = torch.zeros(2, 4, 64, dtype=BF16, device=device, requires_grad=True)
    pool = torch.zeros(4, 2, 16, 64, dtype=BF16, device=device)
    with pytest.raises(RuntimeError, match="inference-only"):
        ops.paged_attention_decode(
            q, pool, pool, torch.zeros(2, 3, dtype=torch.int32, device=device),
            torch.ones(2, dtype=torch.int32, device=device))


_both("paged_attention_arguments", _check_arguments)


def test_paged_num_splits_heuristic():
    """num_splits=0: cover the CUs at small batch*n_kv, keep a few pages
    per split, never below 1."""
    assert ops.paged_num_splits(8, 8, 8192) == 8
    assert ops.paged_num_splits(32, 8, 8192) == 2
    assert ops.paged_num_splits(64, 8, 8192) == 1
    assert ops.paged_num_splits(8, 8, 256) == 1
    assert ops.paged_num_splits(1, 1, 128) == 1
    assert ops.paged_num_splits(1, 8, 1 << 20) == 32


# ---------------------------------------------------------------------------
# paged_kv_write
# ---------------------------------------------------------------------------
def _sentinel_pool(shape):
    n = 1
    for s in shape:
        n *= s
    # finite, all-distinct-looking bf16 bit patterns (exponent byte < 0x7f)
    bits = (torch.arange(n, dtype=torch.int32) * 7 + 3) % 0x3f00
    return bits.to(torch.int16).view(BF16).reshape(shape).clone()


def _check_kv_write(device, hd, Hq, Hkv, ps, T):
    gen = torch.Generator().manual_seed(hd + Hkv + ps + T)
    if T == 1:
        spans = [(ps + 3, 1)]
    else:  # 37 tokens over three sequences, crossing page boundaries
        spans = [(0, 20), (13, 10), (30, 7)]
    table, num_pages = _block_table([s + n for s, n in spans], ps, gen)
    slots = [int(table[b, t // ps]) * ps + t % ps
             for b, (s, n) in enumerate(spans) for t in range(s, s + n)]
    assert len(slots) == T and len(set(slots)) == T
    for skip in ((), (0,)) if T == 1 else ((3, 17, 36),):
        sm = torch.tensor(slots, dtype=torch.int32)
        for i in skip:
            sm[i] = -1
        # k/v as the qkv split gives them: strided views of a wider row
        wide = torch.randn(T, (Hq + 2 * Hkv) * hd, generator=gen).to(BF16)
        wide = wide.to(device)
        k_new = wide[:, Hq * hd:(Hq + Hkv) * hd].view(T, Hkv, hd)
        v_new = wide[:, (Hq + Hkv) * hd:].view(T, Hkv, hd)
        assert not k_new.is_contiguous() or T == 1
        shape = (num_pages, Hkv, ps, hd)
        kp = _sentinel_pool(shape).to(device)
        vp = (-_sentinel_pool(shape)).to(device)
        ref_k, ref_v = kp.clone(), vp.clone()
        keep = sm >= 0
        page, off = (sm[keep] // ps).long(), (sm[keep] % ps).long()
        ref_k[page.to(device), :, off.to(device)] = k_new[keep.to(device)]
        ref_v[page.to(device), :, off.to(device)] = v_new[keep.to(device)]
        ops.paged_kv_write(k_new, v_new, kp, vp, sm.to(device))
        assert torch.equal(_bits(kp), _bits(ref_k)), "k pool differs"
        assert torch.equal(_bits(vp), _bits(ref_v)), "v pool differs"
        if len(skip) == T:
            assert torch.equal(_bits(kp), _bits(_sentinel_pool(shape)))


_both("paged_kv_write", _check_kv_write,
      [(64, 4, 2, 16, 1), (64, 4, 2, 16, 37), (128, 8, 8, 64, 1),
       (128, 8, 8, 64, 37), (128, 8, 1, 32, 37)])


def _check_kv_write_arguments(device):
    pool = torch.zeros(4, 2, 16, 64, dtype=BF16, device=device)
    k = torch.zeros(3, 2, 64, dtype=BF16, device=device)
    sm = torch.zeros(3, dtype=torch.int32, device=device)
    with pytest.raises(RAISES):
        ops.paged_kv_write(k[:, :1], k[:, :1], pool, pool.clone(), sm)
    with pytest.raises(RAISES):
        ops.paged_kv_write(k, k, pool, pool.clone(), sm.long())
    with pytest.raises(RAISES):
        ops.paged_kv_write(k, k, pool, pool.clone(), sm[:2])
    with pytest.raises(RuntimeError, match="inference-only"):
        ops.paged_kv_write(k.clone().requires_grad_(), k, pool, pool.clone(),
                           sm)


_both("paged_kv_write_arguments", _check_kv_write_arguments)
