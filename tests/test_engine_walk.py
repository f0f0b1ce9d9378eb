"""The engine's capturable decode maths, run un-captured on the CPU.

On a GPU `BatchedGenerator._decode_math` only ever runs inside a captured
graph; here it is driven by hand, with `_g_toks`/`_g_act` filled the way
`_decode_graph` fills them, and compared row by row with a second engine
taking the eager step. Both go through `Llama._walk`; what differs is what
the graph path must keep: every slot in the batch (an inactive one
included), lengths advanced by `_g_act`, and for the slot cache the
bucketed horizon read as a view.
"""
import pytest
import torch

from kubetorch_amd.models import BatchedGenerator, Llama, llama_tiny

STEPS = 3
# Slot cache: the full-batch step attends over the bucketed horizon
# (L = 128) and the eager step over max(lens) + 1, so SDPA sums in another
# order. Bound = 4 x the largest |difference| this scenario gives on the
# commit before the engine moved onto Llama._walk (CPU, deterministic):
# fp32 measured 2.3842e-07 -> 9.5367e-07, bf16 measured 3.9062e-03 ->
# 1.5625e-02.
SLOT_BOUND = {torch.float32: 4 * 2.3842e-07, torch.bfloat16: 4 * 3.9062e-03}


def _model(dtype):
    torch.manual_seed(53)
    return Llama(llama_tiny()).eval().to(dtype)


def _engine(model, **kw):
    """Three requests admitted together; the first is done at prefill, so
    slot 0 is inactive for every decode step that follows."""
    eng = BatchedGenerator(model, max_batch=3, graph=False, **kw)
    eng.submit([5, 6, 7], max_new_tokens=1)
    eng.submit(list(range(30, 49)), max_new_tokens=STEPS + 3)   # 19 tokens
    eng.submit([11, 12], max_new_tokens=STEPS + 3)
    eng.step()  # prefill + the first decode step, the same in both engines
    assert [s is not None for s in eng.slots] == [False, True, True]
    return eng


@torch.no_grad()
def _full_batch_step(eng):
    """`_decode_graph` without the graph: {slot: logits}."""
    active = [s for s in range(eng.max_batch) if eng.slots[s] is not None]
    L = None
    if not eng._paged:
        L = eng._bucket_for(max(eng._host_lens[s] for s in active) + 1)
    toks = [0] * eng.max_batch
    act = [0] * eng.max_batch
    for s in active:
        toks[s] = eng.slots[s].next_tok
        act[s] = 1
        eng._host_lens[s] += 1
    eng._g_toks = torch.tensor(toks, dtype=torch.long)
    eng._g_act = torch.tensor(act, dtype=torch.long)
    logits = eng._decode_math(L)
    out = {s: logits[s].clone() for s in active}
    for s in active:
        eng._emit(eng.slots[s], logits[s])
    return out


def _eager_step(eng):
    """One eager `step()`: {slot: logits}, recorded where they are sampled."""
    seen = {}
    sample = eng._sample

    def record(req, logits):
        seen[req.slot] = logits.clone()
        return sample(req, logits)

    eng._sample = record
    try:
        eng.step()
    finally:
        del eng._sample
    return seen


def _run_both(dtype, **kw):
    model = _model(dtype)
    full, eager = _engine(model, **kw), _engine(model, **kw)
    pairs = []
    for _ in range(STEPS):
        a, b = _full_batch_step(full), _eager_step(eager)
        assert sorted(a) == sorted(b) == [1, 2]
        pairs += [(a[s], b[s]) for s in (1, 2)]
        assert full.lens.tolist() == eager.lens.tolist()
        assert full.lens[0] == 0
    toks = [[r.out for r in e.slots if r is not None] for e in (full, eager)]
    return pairs, toks


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
@pytest.mark.parametrize("prefill", ["cache", "paged"])
def test_paged_full_batch_maths_equals_eager_bitwise(prefill, dtype):
    pairs, toks = _run_both(dtype, kv="paged", prefill=prefill)
    for a, b in pairs:
        assert torch.equal(a, b)
    assert toks[0] == toks[1]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
def test_slot_full_batch_maths_matches_eager(dtype):
    pairs, toks = _run_both(dtype)
    worst = max(float((a.float() - b.float()).abs().max()) for a, b in pairs)
    print(f"slot {dtype}: max |full-batch - eager| = {worst:.4e} "
          f"(bound {SLOT_BOUND[dtype]:.4e})")
    assert toks[0] == toks[1]
    assert worst <= SLOT_BOUND[dtype]
