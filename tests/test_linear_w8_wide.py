"""ops.linear_w8 above 32 rows: the 64-row-tile gfx950 kernel.

The contract and the bound are test_linear_w8's (float64 reference,
|y - ref| <= 2^-8 |ref| + K 2^-23 (|x| @ |Wq|^T), derived there); its helpers
are imported, not copied. Shapes: M around the 64-row tile edge, N around the
128-column tile and a wave's 32 columns, K of 2, 3 and 9 tiles (the weight
ring wraps, the LDS double buffer flips). "[edges]" lines report the measured
error over the bound; run with -s.
"""
import pytest
import torch
import torch.nn.functional as F

import test_linear_w8 as tlw
import test_paged_engine as tpe
from kubetorch_amd import ops
from kubetorch_amd.models import BatchedGenerator
from test_linear_w8 import gpu_pair  # noqa: F401  (fixture)

BF16 = torch.bfloat16
NK = ((40, 256), (33, 384), (200, 1152))


def _wide(x, q, s, **kw):
    """ops.linear_w8 on operands the wide kernel must take."""
    assert not ops._linear_w8_kernel_ok(x, q, s)
    assert ops._linear_w8_wide_ok(x, q, s)
    return ops.linear_w8(x, q, s, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("N,K", NK)
@pytest.mark.parametrize("M", (33, 63, 64, 65, 129))
def test_accuracy_f64_gpu(M, N, K):
    q, s, wq64 = tlw._acc_weights(N, K)
    worst = 0.0
    for x in tlw._acc_inputs(M, K, seed=M):
        y = _wide(x.cuda(), q.cuda(), s.cuda())
        assert y.shape == (M, N) and y.dtype == BF16
        worst = max(worst, tlw._ratio(y, x, wq64))
    tlw._note(f"wide accuracy M={M} N={N} K={K}", "cuda", worst)
    assert worst <= 1.0, worst


@pytest.mark.gpu
@pytest.mark.parametrize("N,K", ((128, 2048), (48, 1152)))
def test_split_k_gpu(N, K):
    q, s, wq64 = tlw._weights(N, K, seed=77)
    x = tlw._acc_inputs(65, K, seed=9)[1]
    worst = 0.0
    for S in (1, 2, 3, 8):
        y1 = _wide(x.cuda(), q.cuda(), s.cuda(), num_splits=S)
        y2 = _wide(x.cuda(), q.cuda(), s.cuda(), num_splits=S)
        assert torch.equal(tlw._bits(y1), tlw._bits(y2)), S
        worst = max(worst, tlw._ratio(y1, x, wq64))
    tlw._note(f"wide split-K N={N} K={K}", "cuda", worst)
    assert worst <= 1.0, worst


@pytest.mark.gpu
def test_selection_exact_gpu():
    """A one-hot x selects bf16(Wq[n, k]) bit for bit at every k, in both
    row blocks of the tile: the K permutation."""
    M, N, K = 64, 33, 384
    q, s, wq = tlw._selection_weights(N, K)
    for base in range(0, K, M):
        km = torch.arange(base, base + M) % K
        x = torch.zeros(M, K, dtype=BF16)
        x[torch.arange(M), km] = 1.0
        y = _wide(x.cuda(), q.cuda(), s.cuda()).cpu()
        want = wq[:, km].T.contiguous()
        # bits, except that an all-zero sum may come out as +0 for -0
        same = tlw._bits(y) == tlw._bits(want)
        zero = (want == 0) & (y == 0)
        assert bool((same | zero).all()), (base, (~(same | zero)).nonzero())


@pytest.mark.gpu
@pytest.mark.parametrize("N,K", ((40, 256), (200, 1152)))
def test_rows_are_independent_gpu(N, K):
    q, s, _ = tlw._acc_weights(N, K)
    qd, sd = q.cuda(), s.cuda()
    x = tlw._acc_inputs(129, K, seed=4)[1].cuda()
    y = _wide(x, qd, sd)
    # the same rows at other places of a smaller call, and in the skinny one
    idx = torch.arange(128, -1, -2, device="cuda")  # 65 rows, reversed
    y65 = _wide(x[idx], qd, sd)
    assert torch.equal(tlw._bits(y65), tlw._bits(y[idx]))
    assert ops._linear_w8_kernel_ok(x[idx[:32]], qd, sd)
    y32 = ops.linear_w8(x[idx[:32]], qd, sd)
    assert torch.equal(tlw._bits(y32), tlw._bits(y[idx[:32]]))
    # rows past M are not read
    M = 65
    xbig = torch.full((M + 7, K), float("nan"), dtype=BF16, device="cuda")
    xbig[:M] = x[:M]
    ydead = _wide(xbig[:M], qd, sd)
    assert torch.equal(tlw._bits(ydead), tlw._bits(y[:M]))
    # a column slice with row stride 3K
    wide = torch.full((M, 3 * K), float("nan"), dtype=BF16, device="cuda")
    wide[:, K:2 * K] = x[:M]
    xs = wide[:, K:2 * K]
    assert xs.stride(0) == 3 * K
    assert torch.equal(tlw._bits(_wide(xs, qd, sd)), tlw._bits(y[:M]))


@pytest.mark.gpu
def test_the_path_is_the_kernel_gpu(monkeypatch):
    def boom(*a, **kw):
        raise AssertionError("the composition ran")
    N, K = 40, 256
    q, s, wq64 = tlw._acc_weights(N, K)
    x = tlw._acc_inputs(ops.W8_WIDE_MAX_ROWS + 1, K, seed=2)[0]
    monkeypatch.setattr(ops, "dequantize_weight_fp8", boom)
    y = ops.linear_w8(x[:64].cuda(), q.cuda(), s.cuda())
    assert tlw._ratio(y, x[:64], wq64) <= 1.0
    assert not ops._linear_w8_wide_ok(x.cuda(), q.cuda(), s.cuda())
    with pytest.raises(AssertionError, match="composition"):
        ops.linear_w8(x.cuda(), q.cuda(), s.cuda())


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_engine_wide_decode_graph_matches_eager_gpu(gpu_pair, monkeypatch):
    """36 requests in 40 slots: decode steps of more than 32 rows. Half the
    requests stop early, so eager ends on 18 rows (the skinny kernel) where
    the graph keeps its 40 (the wide one)."""
    qm, dm = gpu_pair
    gen = torch.Generator().manual_seed(17)
    prompts = [torch.randint(0, qm.cfg.vocab_size, (3 + i % 5,),
                             generator=gen).tolist() for i in range(36)]
    calls = []  # (M, taken) of every call the skinny kernel refused
    real = ops._linear_w8_wide_ok

    def spy(x, q, s):
        calls.append((x.numel() // x.shape[-1], real(x, q, s)))
        return calls[-1][1]
    monkeypatch.setattr(ops, "_linear_w8_wide_ok", spy)

    def run(graph):
        eng = BatchedGenerator(qm, max_batch=40, max_len=32, graph=graph,
                               kv="paged", page_size=16)
        rids = [eng.submit(p, max_new_tokens=4 + 4 * (i % 2))
                for i, p in enumerate(prompts)]
        out = eng.run()
        return eng, [out[r] for r in rids]
    _, eager = run(False)
    # every operand of this model is kernel-eligible: only M decides
    assert any(M == 36 and ok for M, ok in calls)
    assert all(ok for M, ok in calls if 32 < M <= ops.W8_WIDE_MAX_ROWS)
    eng, graphed = run(True)
    assert eng._use_graph and eager == graphed
    assert any(M == 40 and ok for M, ok in calls)
    for p, toks in zip(prompts, graphed):
        tpe._assert_teacher_forced(dm, len(p), toks)


def test_cpu_path_is_the_composition():
    q, s, _ = tlw._acc_weights(40, 256)
    x = tlw._acc_inputs(64, 256, seed=3)[0]
    assert not ops._linear_w8_wide_ok(x, q, s)
    want = F.linear(x, ops.dequantize_weight_fp8(q, s, BF16))
    assert torch.equal(tlw._bits(ops.linear_w8(x, q, s)), tlw._bits(want))
