"""ops.paged_attention_prefill: causal GQA attention of a packed,
variable-length batch of query tokens over the paged KV pools.

Same scheme as tests/test_paged_attention.py (helpers copied from there):
every case is a `_check(device, ...)` run on "cpu" against the project's
fp32 reference path and on "cuda" under the gpu marker, where it runs the
gfx950 kernel. Results are compared with a float64 reference built from the
same bf16 inputs under the one-bf16-ulp rule (assert_bf16_ulp).

Tolerance. extra_abs per output element is the fp32 term of
test_paged_attention.py with L = the number of keys the token attends,
(2*(s_max + 4) + L) * 2**-23 * max|v|. The gfx950 kernel rounds P to bf16
for the P.V MFMA (docs/engine.md), so on "cuda" the P-rounding term
2**-8 * (softmax(s) @ |v|), elementwise in float64, is added: RNE of each
p_t is off by at most 2**-8 p_t. The kernel sums l from the unrounded fp32
p, so there is no further 2**-8*|ref| term. The CPU reference path rounds
nothing and gets the fp32 term alone.

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
    Cap: at most 0.1 % of the elements exceed half an ulp,
    2**-8*|ref|*(1 + 2**-10) + extra_abs + floor.
    NaN and inf positions must match the reference exactly.
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


def _gather(pool, table, b, n, ps):
    page = torch.tensor([int(table[b, t // ps]) for t in range(n)])
    off = torch.tensor([t % ps for t in range(n)])
    return _f64(pool[page, :, off]).transpose(0, 1)  # [Hkv, n, hd]


def _reference(q, kp, vp, table, rows, scale):
    """float64 reference [T, Hq, hd] and the two error terms: the fp32 term
    [T, Hq, 1] and the P-rounding term [T, Hq, hd] (module docstring)."""
    T, Hq, hd = q.shape
    Hkv, ps = kp.shape[1], kp.shape[2]
    g = Hq // Hkv
    ref = torch.zeros(T, Hq, hd, dtype=F64)
    e32 = torch.zeros(T, Hq, 1, dtype=F64)
    eP = torch.zeros(T, Hq, hd, dtype=F64)
    t0 = 0
    for b, (ctx, qlen) in enumerate(rows):
        n = ctx + qlen
        if qlen == 0:
            continue
        k = _gather(kp, table, b, n, ps)
        v = _gather(vp, table, b, n, ps)
        qb = _f64(q[t0:t0 + qlen]).view(qlen, Hkv, g, hd).permute(1, 2, 0, 3)
        s = torch.matmul(qb, k.transpose(1, 2).unsqueeze(1)) * scale
        pos = ctx + torch.arange(qlen)
        see = torch.arange(n).view(1, n) <= pos.view(qlen, 1)   # [qlen, n]
        s = s.masked_fill(~see, float("-inf"))       # [Hkv, g, qlen, n]
        p = torch.softmax(s, -1)
        o = torch.matmul(p, v.unsqueeze(1))          # [Hkv, g, qlen, hd]
        oa = torch.matmul(p, v.abs().unsqueeze(1))
        s_max = s.masked_fill(~see, 0.0).abs().amax(-1)          # [Hkv, g, qlen]
        v_max = v.abs().amax(-1).cummax(-1).values[:, pos]       # [Hkv, qlen]
        keys = (pos + 1).to(F64).view(1, 1, qlen)
        f32 = (2 * (s_max + 4) + keys) * 2.0 ** -23 * v_max.unsqueeze(1)
        sl = slice(t0, t0 + qlen)
        ref[sl] = o.permute(2, 0, 1, 3).reshape(qlen, Hq, hd)
        eP[sl] = 2.0 ** -8 * oa.permute(2, 0, 1, 3).reshape(qlen, Hq, hd)
        e32[sl, :, 0] = f32.permute(2, 0, 1).reshape(qlen, Hq)
        t0 += qlen
    return ref, e32, eP


@functools.lru_cache(maxsize=None)
def _case(hd, Hq, Hkv, ps, rows, seed=0):
    """rows: ((ctx, qlen), ...). q is a strided view of a wider row, as the
    qkv split gives it."""
    gen = torch.Generator().manual_seed(1000 * seed + 7 * hd + Hq + Hkv + ps)
    seq_lens = [c + n for c, n in rows]
    table, num_pages = _block_table(seq_lens, ps, gen)
    shape = (num_pages, Hkv, ps, hd)
    T = sum(n for _, n in rows)
    wide = (torch.randn(T, (Hq + 2 * Hkv) * hd, generator=gen) * 1.5).to(BF16)
    q = wide[:, :Hq * hd].view(T, Hq, hd)
    kp = torch.randn(shape, generator=gen).to(BF16)
    vp = torch.randn(shape, generator=gen).to(BF16)
    cu = [0]
    for _, n in rows:
        cu.append(cu[-1] + n)
    scale = hd ** -0.5
    ref, e32, eP = _reference(q, kp, vp, table, rows, scale)
    return dict(q=q, wide=wide, kp=kp, vp=vp, table=table, rows=rows,
                cu=torch.tensor(cu, dtype=torch.int32),
                lens=torch.tensor(seq_lens, dtype=torch.int32),
                max_q=max(n for _, n in rows), ref=ref, e32=e32, eP=eP,
                valid=_valid_mask(table, seq_lens, num_pages, ps),
                scale=scale)


def _extra(device, c):
    """The P-rounding term is allowed only where P is rounded: the kernel."""
    return c["e32"] + c["eP"] if device == "cuda" else c["e32"].expand_as(c["eP"])


def _run(device, c, q=None, kp=None, vp=None, lens=None, cu=None, table=None,
         max_q=None):
    Hq, hd = c["q"].shape[1:]
    if q is None:
        wide = c["wide"].to(device)
        q = wide[:, :Hq * hd].view(-1, Hq, hd)
        assert not q.is_contiguous() or q.shape[0] == 1
    kp = c["kp"] if kp is None else kp
    vp = c["vp"] if vp is None else vp
    lens = c["lens"] if lens is None else lens
    cu = c["cu"] if cu is None else cu
    table = c["table"] if table is None else table
    return ops.paged_attention_prefill(
        q.to(device), kp.to(device), vp.to(device), table.to(device),
        cu.to(device), lens.to(device), c["max_q"] if max_q is None else max_q)


def _report(name, out, c, extra):
    err = (_f64(out).cpu() - c["ref"]).abs()
    bound = 2.0 ** -7 * c["ref"].abs() + extra + 1e-30
    _note(name + "_max_abs_err", err.max().item())
    _note(name + "_max_err_over_bound", (err / bound).max().item())


def _ragged_rows(ps):
    # single token; page crossing from scratch; one token after a full page;
    # page boundary between context and query; several key tiles with the
    # query spilling past a 64-row tile; diagonal tiles and tile skipping;
    # a row without query tokens
    return ((0, 1), (0, ps + 1), (ps, 1), (ps - 1, 2), (3 * 64 + 5, 70),
            (0, 130), (5, 0))


def _check_ragged(device, hd, Hq, Hkv, ps):
    c = _case(hd, Hq, Hkv, ps, _ragged_rows(ps))
    out = _run(device, c)
    name = f"prefill_ragged_{device}_hd{hd}_q{Hq}_kv{Hkv}_ps{ps}"
    assert out.dtype == BF16 and out.shape == c["q"].shape
    assert out.is_contiguous()
    extra = _extra(device, c)
    _report(name, out, c, extra)
    assert bool(out.isfinite().all()), name
    assert_bf16_ulp(out, c["ref"], extra, msg=name)


_both("paged_prefill_ragged", _check_ragged, CASES)


def _check_decode_agreement(device, hd, Hq, Hkv, ps):
    """qlen = 1 rows are the decode op's case: same inputs, results within
    twice the bound (different summation orders, no bitwise claim)."""
    rows = ((0, 1), (ps - 1, 1), (ps, 1), (3 * 64 + 5, 1), (599, 1))
    c = _case(hd, Hq, Hkv, ps, rows)
    out = _run(device, c)
    extra = _extra(device, c)
    assert_bf16_ulp(out, c["ref"], extra, msg="prefill qlen=1")
    dec = ops.paged_attention_decode(
        c["q"].contiguous().to(device), c["kp"].to(device), c["vp"].to(device),
        c["table"].to(device), c["lens"].to(device), num_splits=1)
    diff = (_f64(out) - _f64(dec)).abs().cpu()
    twice = 2 * (2.0 ** -7 * c["ref"].abs() + extra)
    _note(f"prefill_vs_decode_{device}_hd{hd}_q{Hq}_kv{Hkv}_ps{ps}",
          (diff / (twice + 1e-30)).max().item())
    assert bool((diff <= twice).all()), "prefill and decode disagree"


_both("paged_prefill_decode_agreement", _check_decode_agreement, CASES)


def _poisoned(c, value):
    """K and V with `value` at every position that holds no valid token:
    all of every page the table does not reference, and positions >=
    seq_len of each last page."""
    dead = ~c["valid"][:, None, :, None]
    fill = torch.tensor(value, dtype=BF16)
    return (torch.where(dead, fill, c["kp"]), torch.where(dead, fill, c["vp"]))


def _check_poison(device, hd, Hq, Hkv, ps):
    c = _case(hd, Hq, Hkv, ps, _ragged_rows(ps))
    kp, vp = _poisoned(c, 0.0)
    clean = _run(device, c, kp=kp, vp=vp)
    assert_bf16_ulp(clean, c["ref"], _extra(device, c), msg="zeroed baseline")
    for value in (float("nan"), float("inf")):
        kp, vp = _poisoned(c, value)
        assert not bool(kp.isfinite().all())
        out = _run(device, c, kp=kp, vp=vp)
        assert torch.equal(_bits(out), _bits(clean)), \
            f"poison {value} reached the output"


_both("paged_prefill_poison", _check_poison, CASES)


def _check_causality(device, hd, Hq, Hkv, ps):
    """Other finite q rows and K/V at positions > t leave the outputs of
    tokens at positions <= t bitwise unchanged (t is mid-query per row)."""
    c = _case(hd, Hq, Hkv, ps, _ragged_rows(ps))
    base = _run(device, c)
    gen = torch.Generator().manual_seed(99)
    q = c["q"].clone()
    kp, vp = c["kp"].clone(), c["vp"].clone()
    keep = torch.zeros(q.shape[0], dtype=torch.bool)
    t0 = 0
    for b, (ctx, qlen) in enumerate(c["rows"]):
        t = ctx + qlen // 2 - 1     # last position that must not change
        for i in range(qlen):
            if ctx + i <= t:
                keep[t0 + i] = True
            else:
                q[t0 + i] = (torch.randn(q.shape[1:], generator=gen) * 3).to(BF16)
        for pos in range(max(t + 1, 0), ctx + qlen):
            pg = int(c["table"][b, pos // ps])
            kp[pg, :, pos % ps] = (torch.randn(Hkv, hd, generator=gen) * 3).to(BF16)
            vp[pg, :, pos % ps] = (torch.randn(Hkv, hd, generator=gen) * 3).to(BF16)
        t0 += qlen
    assert bool(keep.any()) and not bool(keep.all())
    out = _run(device, c, q=q, kp=kp, vp=vp)
    assert torch.equal(_bits(out[keep]), _bits(base[keep])), \
        "a token saw a later position"
    assert not torch.equal(_bits(out[~keep]), _bits(base[~keep]))


_both("paged_prefill_causality", _check_causality,
      [(64, 4, 2, 16), (128, 8, 2, 64), (128, 8, 1, 16)])


def _check_chunks(device, hd, Hq, Hkv, ps):
    """A 70-token prompt in one call, and as 40 tokens followed by 30 with
    ctx = 40 (K/V of all 70 are in the pages either way)."""
    c = _case(hd, Hq, Hkv, ps, ((0, 70),))
    whole = _run(device, c)
    extra = _extra(device, c)
    assert_bf16_ulp(whole, c["ref"], extra, msg="whole prompt")
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    first = _run(device, c, q=c["q"][:40], lens=i32(40), cu=i32(0, 40),
                 max_q=40)
    second = _run(device, c, q=c["q"][40:], lens=i32(70), cu=i32(0, 30),
                  max_q=30)
    parts = torch.cat([first, second])
    assert_bf16_ulp(parts, c["ref"], extra, msg="two chunks")
    diff = (_f64(parts) - _f64(whole)).abs().cpu()
    twice = 2 * (2.0 ** -7 * c["ref"].abs() + extra)
    assert bool((diff <= twice).all()), "chunked and whole prefill disagree"


_both("paged_prefill_chunks", _check_chunks, CASES)


def _check_deterministic(device):
    c = _case(128, 8, 2, 16, _ragged_rows(16))
    a, b = _run(device, c), _run(device, c)
    assert torch.equal(_bits(a), _bits(b)), "not deterministic"


_both("paged_prefill_deterministic", _check_deterministic)


def _check_bad_rows(device, hd, Hq, Hkv, ps):
    """A row with more query tokens than seq_lens, and a row whose
    positions lie beyond max_blocks*page_size, give zero rows; a row that
    crosses the table's capacity is zero from there on. The other rows'
    results are bitwise unchanged."""
    rows = ((0, 20), (10, 5), (3, 9), (ps, 6))
    c = _case(hd, Hq, Hkv, ps, rows)
    base = _run(device, c)
    assert_bf16_ulp(base, c["ref"], _extra(device, c), msg="bad rows baseline")
    cap = c["table"].shape[1] * ps
    lens = c["lens"].clone()
    lens[1] = 3            # qlen 5 > seq_len 3
    lens[2] = cap + 20     # every position of the row >= cap
    out = _run(device, c, lens=lens)
    assert int(_bits(out[20:34]).count_nonzero()) == 0, "bad rows not zero"
    assert torch.equal(_bits(out[:20]), _bits(base[:20]))
    assert torch.equal(_bits(out[34:]), _bits(base[34:]))
    # row 3 with its last 2 of 6 tokens past the capacity: a full table row
    table = c["table"].clone()
    spare = [p for p in range(c["kp"].shape[0])
             if p not in set(c["table"].reshape(-1).tolist())]
    nb = table.shape[1]
    used = _pages_for(ps + 6, ps)
    table[3, used:] = torch.tensor(spare[:nb - used], dtype=torch.int32)
    lens = c["lens"].clone()
    lens[3] = cap + 2
    out = _run(device, c, lens=lens, table=table)
    assert bool(out.isfinite().all())
    assert int(_bits(out[38:]).count_nonzero()) == 0, "tokens past the table"
    assert int(_bits(out[34:38]).count_nonzero()) > 0
    assert torch.equal(_bits(out[:34]), _bits(base[:34]))
    # tokens at index >= cu[B] stay zero
    out = _run(device, c, cu=c["cu"][:3], lens=c["lens"][:2],
               table=c["table"][:2])
    assert int(_bits(out[25:]).count_nonzero()) == 0
    assert torch.equal(_bits(out[:25]), _bits(base[:25]))


_both("paged_prefill_bad_rows", _check_bad_rows,
      [(64, 4, 2, 16), (128, 8, 2, 64)])


def _check_arguments(device):
    """Unsupported configurations raise; on the GPU these stop at the
    host-side checks, nothing is launched."""
    def call(hd=64, Hq=4, Hkv=2, ps=16, qdtype=BF16, pool=None, cu=None,
             lens=None):
        q = torch.zeros(3, Hq, hd, dtype=qdtype, device=device)
        if pool is None:
            pool = torch.zeros(4, Hkv, ps, hd, dtype=BF16, device=device)
        table = torch.zeros(2, 3, dtype=torch.int32, device=device)
        if cu is None:
            cu = torch.tensor([0, 1, 3], dtype=torch.int32, device=device)
        if lens is None:
            lens = torch.tensor([1, 2], dtype=torch.int32, device=device)
        return ops.paged_attention_prefill(
            q, pool, pool.clone() if pool.is_contiguous() else pool, table,
            cu.to(device), lens.to(device), 2)

    assert call().shape == (3, 4, 64)  # the supported form of the same call
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
    with pytest.raises(RAISES):
        call(cu=torch.tensor([0, 1, 3]))
    with pytest.raises(RAISES):
        call(lens=torch.tensor([1, 2]))
    with pytest.raises(RAISES):
        call(cu=torch.tensor([0, 1, 3, 3], dtype=torch.int32))
    q = torch.zeros(3, 4, 64, dtype=BF16, device=device, requires_grad=True)
    pool = torch.zeros(4, 2, 16, 64, dtype=BF16, device=device)
    with pytest.raises(RuntimeError, match="inference-only"):
        ops.paged_attention_prefill(
            q, pool, pool, torch.zeros(2, 3, dtype=torch.int32, device=device),
            torch.tensor([0, 1, 3], dtype=torch.int32, device=device),
            torch.tensor([1, 2], dtype=torch.int32, device=device), 2)


_both("paged_prefill_arguments", _check_arguments)
