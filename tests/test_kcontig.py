"""K-contiguous backward operands: the bf16 transpose kernels, ops.linear /
ops.Linear, and the FlatDDP W^T shadows with their freshness stamps."""
import pytest
import torch
import torch.nn.functional as F

from kubetorch_amd import ops
from kubetorch_amd.models import Llama, llama_tiny
from kubetorch_amd.parallel import FlatDDP
from kubetorch_amd.utils import checkpoint as ckpt

# Margin between two bf16 summation orders. Measured on the shapes used
# below (T=256, (in,out) in {(128,192),(136,72)}, 20 seeds, y/dX/dW): the
# max-abs error against fp64 (relative to the result's max-abs) of a GEMM
# whose K loop is split in two with the partial sums rounded to bf16 is up
# to 2.37x that of the single fp32-accumulated GEMM on the same inputs
# (1.91x .. 2.37x over the six cases); a pure permutation of K with fp32
# accumulation gives 1.000x, because the final bf16 rounding dominates.
# 2.5 is that observation rounded up.
ORDER_MARGIN = 2.5
BF16_EPS = 2.0 ** -8


# ---------------------------------------------------------------------------
# transpose kernels
# ---------------------------------------------------------------------------
def _rand_bf16(shape, device, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).bfloat16().to(device)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(8, 8), (64, 64), (72, 136), (8, 4104),
                                   (4104, 24)])
def test_transpose_bitwise(shape):
    src = _rand_bf16(shape, "cuda", 1)
    assert ops._transpose_kernel_ok(src)  # the kernel, not the fallback
    dst = ops.transpose_bf16(src)
    assert dst.shape == (shape[1], shape[0]) and dst.is_contiguous()
    assert torch.equal(dst, src.t().contiguous())


@pytest.mark.gpu
def test_transpose_strided_source():
    wide = _rand_bf16((200, 192), "cuda", 2)
    src = wide[:, 64:128]
    assert src.stride(0) == 192 and ops._transpose_kernel_ok(src)
    assert torch.equal(ops.transpose_bf16(src), src.t().contiguous())


def test_transpose_fallbacks_cpu():
    a = _rand_bf16((12, 20), "cpu", 3)       # not multiples of 8, CPU
    assert torch.equal(ops.transpose_bf16(a), a.t().contiguous())
    f = torch.randn(16, 8)
    assert torch.equal(ops.transpose_bf16(f), f.t().contiguous())


def _segment_layout():
    """A flat buffer with 1-D segments (no table entry) around three 2-D
    segments; (8, 16) is smaller than one 64x64 tile, (72, 136) is ragged
    in both dimensions, (128, 64) is exact tiles."""
    layout = [("vec", 24), ("mat", (72, 136)), ("vec", 8), ("mat", (8, 16)),
              ("mat", (128, 64)), ("vec", 40)]
    segs, off, toff = [], 0, 16   # dst starts with 16 untouched elements
    for kind, shp in layout:
        if kind == "mat":
            segs.append((off, toff, shp[0], shp[1]))
            off += shp[0] * shp[1]
            toff += shp[0] * shp[1] + 8   # a gap after every dst segment
        else:
            off += shp
    return segs, off, toff


def _check_segments(device):
    segs, n_src, n_dst = _segment_layout()
    src = _rand_bf16((n_src,), device, 4)
    dst = _rand_bf16((n_dst,), device, 5)
    before = dst.clone()
    table, max_tiles = ops.transpose_table(segs, n_src, n_dst, device)
    assert max_tiles == 2 * 3
    ops.transpose_segments_bf16(src, dst, table, max_tiles)
    untouched = torch.ones(n_dst, dtype=torch.bool, device=device)
    for so, do, r, c in segs:
        want = src[so:so + r * c].view(r, c).t().contiguous().reshape(-1)
        assert torch.equal(dst[do:do + r * c], want)
        untouched[do:do + r * c] = False
    assert untouched.sum() == 16 + 8 * 3
    assert torch.equal(dst[untouched], before[untouched])


def test_transpose_segments_cpu():
    _check_segments("cpu")


@pytest.mark.gpu
def test_transpose_segments_gpu():
    _check_segments("cuda")


def test_transpose_table_rejects_bad_segments():
    with pytest.raises(ValueError):
        ops.transpose_table([(0, 0, 8, 16)], 127, 128, "cpu")   # src OOB
    with pytest.raises(ValueError):
        ops.transpose_table([(0, 8, 8, 16)], 128, 128, "cpu")   # dst OOB
    with pytest.raises(ValueError):
        ops.transpose_table([(0, 0, 8, 12)], 128, 128, "cpu")   # cols % 8
    with pytest.raises(ValueError):
        ops.transpose_table([(0, 0, 8, 8), (64, 32, 8, 8)], 128, 128, "cpu")


# ---------------------------------------------------------------------------
# ops.linear
# ---------------------------------------------------------------------------
_T = 256
_LINEAR_SHAPES = [(128, 192), (136, 72)]
_LINEAR_CASES = {}


def _linear_case(in_f, out_f, device):
    """Inputs, the fp64 autograd reference and the plain bf16 F.linear
    errors, computed once per (shape, device) and shared."""
    key = (in_f, out_f, device)
    if key in _LINEAR_CASES:
        return _LINEAR_CASES[key]
    g = torch.Generator().manual_seed(in_f * 1000 + out_f)
    x = torch.randn(2, _T // 2, in_f, generator=g).bfloat16().to(device)
    w = (torch.randn(out_f, in_f, generator=g) * 0.05).bfloat16().to(device)
    dy = torch.randn(2, _T // 2, out_f, generator=g).bfloat16().to(device)
    xd = x.double().requires_grad_()
    wd = w.double().requires_grad_()
    yd = F.linear(xd, wd)
    yd.backward(dy.double())
    ref = {"y": yd.detach(), "dx": xd.grad, "dw": wd.grad}
    xp = x.clone().requires_grad_()
    wp = w.clone().requires_grad_()
    yp = F.linear(xp, wp)
    yp.backward(dy)
    plain = _errors({"y": yp.detach(), "dx": xp.grad, "dw": wp.grad}, ref)
    _LINEAR_CASES[key] = (x, w, dy, ref, plain)
    return _LINEAR_CASES[key]


def _errors(got, ref):
    return {k: ((got[k].double() - ref[k]).abs().max()
                / ref[k].abs().max()).item() for k in ref}


def _run_linear(x, w, dy, with_t, wgrad):
    xq = x.clone().requires_grad_()
    wq = w.clone().requires_grad_()
    wt = ops.make_weight_t(wq) if with_t else None
    y = ops.linear(xq, wq, wt, wgrad=wgrad)
    y.backward(dy)
    return {"y": y.detach(), "dx": xq.grad, "dw": wq.grad}, wt


def _check_linear(device):
    for in_f, out_f in _LINEAR_SHAPES:
        x, w, dy, ref, plain = _linear_case(in_f, out_f, device)
        for with_t in (False, True):
            for wgrad in ops.WGRAD_VARIANTS:
                got, _ = _run_linear(x, w, dy, with_t, wgrad)
                assert got["dx"].shape == x.shape
                assert got["dw"].shape == w.shape
                err = _errors(got, ref)
                print(f"{device} ({in_f},{out_f}) weight_t={with_t} "
                      f"wgrad={wgrad}: err={err} plain={plain}")
                for k in err:
                    assert err[k] <= ORDER_MARGIN * plain[k], (
                        k, in_f, out_f, with_t, wgrad, err[k], plain[k])


def test_linear_vs_fp64_cpu():
    _check_linear("cpu")


@pytest.mark.gpu
def test_linear_vs_fp64_gpu():
    _check_linear("cuda")


def _check_stale(device):
    x, w, dy, _, _ = _linear_case(128, 192, device)
    xq = x.clone().requires_grad_()
    wq = w.clone().requires_grad_()
    wt = ops.make_weight_t(wq)
    assert ops.weight_t_is_fresh(wt, wq)
    with torch.no_grad():
        wq.mul_(-2.0)                   # the shadow now holds the OLD weight
    assert not ops.weight_t_is_fresh(wt, wq)
    ops.linear(xq, wq, wt).backward(dy)
    xr = x.clone().requires_grad_()
    F.linear(xr, wq.detach()).backward(dy)
    assert torch.equal(xq.grad, xr.grad)
    # an engine-side write (no autograd version bump) is caught by the clock
    clock = ops.ShadowClock()
    wt2 = ops.make_weight_t(wq, clock)
    assert ops.weight_t_is_fresh(wt2, wq)
    clock.value = (1, 1)
    assert not ops.weight_t_is_fresh(wt2, wq)
    # an unstamped tensor is never trusted
    assert not ops.weight_t_is_fresh(wq.detach().t().contiguous(), wq)


def test_stale_weight_t_cpu():
    _check_stale("cpu")


@pytest.mark.gpu
def test_stale_weight_t_gpu():
    _check_stale("cuda")


def test_linear_no_grad_and_module():
    lin = ops.Linear(16, 24)
    assert [n for n, _ in lin.named_parameters()] == ["weight"]
    assert list(lin.state_dict()) == ["weight"] and not list(lin.buffers())
    x = torch.randn(4, 16)
    with torch.no_grad():
        assert torch.equal(lin(x), F.linear(x, lin.weight))
    with pytest.raises(ValueError):
        ops.Linear(16, 24, bias=True)


# ---------------------------------------------------------------------------
# engine
# ---------------------------------------------------------------------------
_LR = 1e-3
_STEPS = 3


def _tiny(device="cpu", seed=0, **engine_kw):
    torch.manual_seed(seed)
    cfg = llama_tiny(n_layers=2, dim=128, intermediate=256, vocab_size=256,
                     n_heads=4, n_kv_heads=2)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with torch.device(device):
            model = Llama(cfg)
    finally:
        torch.set_default_dtype(prev)
    eng = FlatDDP(model, lr=_LR, bucket_mb=0.25, **engine_kw)
    g = torch.Generator().manual_seed(7)
    x = torch.randint(0, cfg.vocab_size, (2, 32), generator=g).to(device)
    y = torch.randint(0, cfg.vocab_size, (2, 32), generator=g).to(device)
    return model, eng, x, y


def _linears(model):
    return [m for m in model.modules() if isinstance(m, ops.Linear)]


def _assert_shadows_exact(model):
    mods = _linears(model)
    assert len(mods) == 4 * len(model.layers) + 1
    for m in mods:
        assert m.weight_t is not None
        assert torch.equal(m.weight_t, m.weight.detach().t())
        assert ops.weight_t_is_fresh(m.weight_t, m.weight)


def _train(eng_kw, shadows, micro=1):
    model, eng, x, y = _tiny(transposed_shadows=shadows, **eng_kw)
    for _ in range(_STEPS):
        for _ in range(micro):
            model.loss(x, y).backward()
        eng.step()
        if shadows:
            _assert_shadows_exact(model)
    return torch.cat([b.flat_param.float().reshape(-1) for b in eng.buckets])


@pytest.mark.parametrize("mode", ["overlap_off", "clip_norm", "grad_accum"])
def test_engine_shadows_match_plain_cpu(mode):
    kw = {"overlap_off": dict(overlap_optimizer=False),
          "clip_norm": dict(clip_norm=0.5),
          "grad_accum": dict(grad_accum_steps=2)}[mode]
    micro = 2 if mode == "grad_accum" else 1
    on = _train(kw, True, micro)
    off = _train(kw, False, micro)
    diff = (on - off).abs()
    # Worst case per element and step: AdamW's normalised update is at most
    # lr in magnitude, so a gradient perturbed within the matmul-order
    # margin can at most flip it (2*lr); on top, the bf16 store of the
    # param can land one ulp apart.
    ulp = off.abs().clamp(min=2.0 ** -126) * BF16_EPS
    assert bool((diff <= _STEPS * (2 * _LR + ulp)).all()), diff.max()
    # and overall the two runs differ by no more than bf16 rounding of the
    # params times the summation-order margin
    rel = diff.norm() / off.norm()
    print(f"{mode}: max diff {diff.max():.3e} rel L2 {rel:.3e}")
    assert rel <= ORDER_MARGIN * BF16_EPS


def test_engine_shadows_follow_every_writer_cpu(tmp_path):
    model, eng, x, y = _tiny(transposed_shadows=True,
                             overlap_optimizer=False)
    assert eng.shadows_enabled
    _assert_shadows_exact(model)                       # construction
    model.loss(x, y).backward()
    eng.step()
    _assert_shadows_exact(model)                       # step()
    sd = {k: (v.clone() if torch.is_tensor(v) else
              [t.clone() for t in v] if isinstance(v, list) else v)
          for k, v in eng.state_dict().items()}
    path = str(tmp_path / "ck.pt")
    ckpt.save_engine_checkpoint(model, eng, path)
    model.loss(x, y).backward()
    eng.step()
    with torch.no_grad():                              # an outside writer
        for b in eng.buckets:
            b.flat_param.mul_(0.5)
    lin = _linears(model)[0]
    assert not torch.equal(lin.weight_t, lin.weight.detach().t())
    eng.refresh_transposed()
    _assert_shadows_exact(model)                       # refresh_transposed()
    eng.load_state_dict(sd)
    _assert_shadows_exact(model)                       # load_state_dict
    assert torch.equal(eng.buckets[0].flat_param, sd["flat_param"][0])
    with torch.no_grad():
        for b in eng.buckets:
            b.flat_param.add_(1.0)
    eng.broadcast_params()
    _assert_shadows_exact(model)                       # broadcast_params
    ckpt.load_engine_checkpoint(model, eng, path)
    _assert_shadows_exact(model)                       # checkpoint restore


def test_engine_stale_shadow_not_used_cpu():
    """A write the engine was told about but that has not been followed by
    a refresh leaves every shadow stale, and backward gives the plain
    path's gradients."""
    model, eng, x, y = _tiny(transposed_shadows=True,
                             overlap_optimizer=False)
    ref_model, ref_eng, _, _ = _tiny(transposed_shadows=False,
                                     overlap_optimizer=False)
    for e in (eng, ref_eng):
        e.mark_params_written()
        with torch.no_grad():
            for b in e.buckets:
                b.flat_param.mul_(-1.5)
    for m in _linears(model):
        assert not ops.weight_t_is_fresh(m.weight_t, m.weight)
    model.loss(x, y).backward()
    ref_model.loss(x, y).backward()
    for b, rb in zip(eng.buckets, ref_eng.buckets):
        assert torch.equal(b.flat_grad, rb.flat_grad)


def test_engine_flag_and_env_switch(monkeypatch):
    model, eng, _, _ = _tiny()                 # CPU default: off
    assert not eng.shadows_enabled
    assert all(m.weight_t is None for m in _linears(model))
    monkeypatch.setenv("KT_KCONTIG", "0")
    model, eng, _, _ = _tiny(transposed_shadows=True)
    assert not eng.shadows_enabled
    assert all(m.weight_t is None for m in _linears(model))


def test_state_dict_keys_and_convert():
    from kubetorch_amd.models import convert

    cfg = llama_tiny(n_layers=2, dim=128, intermediate=256, vocab_size=256,
                     n_heads=4, n_kv_heads=2)
    model = Llama(cfg)
    keys = set(model.state_dict())
    want = {"embed.weight", "norm.weight", "lm_head.weight"}
    for i in range(cfg.n_layers):
        want |= {f"layers.{i}.{n}.weight" for n in (
            "attn.wqkv", "attn.wo", "mlp.w_gate_up", "mlp.w_down",
            "attn_norm", "mlp_norm")}
    assert keys == want
    hf = convert.kt_to_hf_state_dict(model.state_dict(), cfg)
    back = convert.hf_to_kt_state_dict(hf, cfg)
    with torch.device("meta"):
        fresh = Llama(cfg)
    fresh = fresh.to_empty(device="cpu")       # load_hf_checkpoint's route
    missing, unexpected = fresh.load_state_dict(back, strict=False)
    assert not unexpected
    assert [m for m in missing if not m.startswith("rope_")] == []
    for k, v in model.state_dict().items():
        assert torch.equal(fresh.state_dict()[k], v)
    # an engine on top leaves the names alone too
    FlatDDP(fresh, bucket_mb=0.25, transposed_shadows=True)
    assert set(fresh.state_dict()) == want


@pytest.mark.gpu
def test_engine_shadows_overlap_gpu():
    model, eng, x, y = _tiny(device="cuda")
    assert eng.shadows_enabled and eng._overlap
    assert any(b.t_table is not None for b in eng.buckets)
    _assert_shadows_exact(model)
    for _ in range(2):
        model.loss(x, y).backward()
        eng.step()
    torch.cuda.synchronize()
    _assert_shadows_exact(model)
