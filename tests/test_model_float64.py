"""The dense Llama as a whole against a float64 reference.

The op suites (test_ops_edges.py, test_attention_dense.py, test_attn_pack.py,
test_kcontig.py, ...) hold every fused op to float64 on its own. This file
holds what `Llama` computes once it wires them together: the loss, every
parameter gradient and the logits, on every attention route, through the
checkpointed walk, through the FlatDDP engine and through the KV cache.

`ref(state_dict, cfg, tokens, targets, dtype)` is a plain-torch Llama that
imports nothing from kubetorch_amd.ops. It runs twice on the same
bf16-rounded weights:

  * dtype=float64 is the reference;
  * dtype=bfloat16 is the NAIVE BASELINE, the same composition with every
    intermediate rounded to bf16. It is not the code under test; it measures
    how much bf16 noise this input carries.

The rule, for every gradient tensor g (wqkv.grad cut into its q, k and v
rows, 19 tensors in all) with reference r and baseline b:

  noise  ||g - r|| / ||r||  <=  margin * ||b - r|| / ||r||,  margin = 1.0:
         the fused kernels exist to round less often than the naive
         composition, so being noisier than it is a finding;
  bias   |<g - r, r> / <r, r>|  <=  2 * max over slices |<b - r, r> / <r, r>|:
         a systematic scale error does not average out of this term; the
         factor 2 is there because the bound is a maximum of 19 noisy
         statistics;
  loss   |loss - loss64| <= 2**-7 * max|logits64|: half a bf16 ulp of the
         target logit plus half an ulp inside the log-sum-exp is
         2**-8 * max|logit|, the same again covers everything upstream;
  no NaN and no inf anywhere.

For logits: every [vocab] row's relative L2 error is at most the baseline's
WORST row error on the same input, and the whole tensor obeys the noise and
bias rules.

The model (`_weights("big")`) is the smallest that opens the v3, ck and wmma
gates (hd = 128). Its q and k rows are redrawn with std 0.06 and its norm
weights with 1 + 0.25*randn: with the default init the scaled scores have a
standard deviation near 0.2, attention is close to uniform and almost no
gradient flows through q and k, so a model-level test could not see the q/k
half of attn_grad_pack, the v3 q scale or the RoPE backward. 37 targets are
-100, so n_valid != B*S.

Every case is a `_check(device, ...)` run on "cpu" against the project's CPU
reference path (which proves the rule and its margins on any machine) and on
"cuda" under the gpu marker, where it runs the gfx950 kernels. Spies on
ops.qkv_attention, ops.flash_attention, Attention._sdpa, the extension's
entry points and the autograd graph assert that a GPU case took the route it
names. test_rule_catches_wrong_models proves that the rule can fail.

Lines starting with "[edges]" report the worst measured ratios; run with -s.
Worst ratios measured (noise = share of the baseline's noise, limit 1.0;
bias = share of the bias bound, limit 1.0; loss = share of the loss bound):

  training         MI355X: noise  bias   loss     CPU path: noise  bias   loss
  v3                       0.561  0.338  0.0033             0.560  0.236  0.0081
  ck (S=384)               0.554  0.194  0.0112             0.554  0.333  0.0019
  wmma                     0.567  0.326  0.0028             0.581  0.216  0.0110
  sdpa                     0.561  0.276  0.0074             0.581  0.216  0.0110
  odd_s (S=200)            0.569  0.313  0.0016             0.578  0.267  0.0149
  unpacked                 0.561  0.397  0.0033             0.581  0.216  0.0110
  ck_backward              0.561  0.341  0.0033             0.581  0.216  0.0110
  checkpointed             0.561  0.338  0.0033             0.581  0.216  0.0110
  kcontig_off              0.561  0.338  0.0033             0.581  0.216  0.0110
  engine                   0.561  0.354  0.0033             0.581  0.216  0.0110
  accumulate               0.579  0.678  0.0198             0.599  0.466  0.0110
  wgrad_layouts            0.561  0.338  0.0033             0.581  0.216  0.0110

  logits           MI355X: row    noise  bias     CPU path: row    noise  bias
  full_256                 0.497  0.569  0.606              0.474  0.565  0.349
  full_200                 0.424  0.567  0.313              0.455  0.564  0.242
  kv_cache                 0.470  0.528  0.128              0.437  0.512  0.123
  llama_tiny forward       0.797  0.846  0.132   (tests/test_model.py)
  llama_tiny cache, worst  0.635  0.906  0.194   (tests/test_model.py)

No route needed a margin of its own. On the CPU every case but v3 and ck is
the same rope + SDPA computation, hence the equal figures.
"""
import collections
import functools

import pytest
import torch
import torch.nn.functional as F

from kubetorch_amd import ops
from kubetorch_amd.models import KVCache, Llama, LlamaConfig, llama_tiny
from kubetorch_amd.models.llama import Attention
from kubetorch_amd.parallel import FlatDDP

BF16 = torch.bfloat16
F64 = torch.float64

CFG = LlamaConfig(dim=512, n_layers=2, n_heads=4, n_kv_heads=2,
                  intermediate=1024, vocab_size=512, max_seq_len=512)
B = 2
ENV = ("KT_ATTN", "KT_ATTN_PACK", "KT_ATTN_BWD", "KT_KCONTIG")

# noise margin per route. 1.0 everywhere: a route gets its own (capped at 2)
# only where the code of a named op shows that it rounds more often than the
# naive composition.
NOISE_MARGIN = collections.defaultdict(lambda: 1.0)


def _note(name, value):
    print(f"[edges] {name} {value:.3e}")


def _both(name, check, cases):
    """Register test_<name>_cpu (unmarked) and test_<name>_gpu (gpu)."""
    par = pytest.mark.parametrize("case", cases)

    @par
    def cpu(case, monkeypatch):
        check("cpu", case, monkeypatch)

    @par
    def gpu(case, monkeypatch):
        check("cuda", case, monkeypatch)
    gpu = pytest.mark.gpu(gpu)
    for fn, suffix in ((cpu, "cpu"), (gpu, "gpu")):
        fn.__name__ = fn.__qualname__ = f"test_{name}_{suffix}"
        globals()[fn.__name__] = fn


# ---------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------
def ref(state_dict, cfg, tokens, targets, dtype):
    """Plain dense Llama in `dtype` -> (loss, {name: grad}, logits); with
    targets None only the logits are computed. Every torch op rounds its
    result to `dtype`, so bfloat16 gives the naive baseline."""
    train = targets is not None
    P = {k: v.detach().to(dtype).requires_grad_(train)
         for k, v in state_dict.items()}
    Bt, S = tokens.shape
    hd, Hq, Hkv = cfg.head_dim, cfg.n_heads, cfg.n_kv_heads
    inv_freq = 1.0 / cfg.rope_base ** (
        torch.arange(0, hd, 2, dtype=F64) / hd)
    ang = torch.outer(torch.arange(S, dtype=F64), inv_freq)
    cos = torch.cat([ang.cos(), ang.cos()], -1).to(dtype).view(1, S, 1, hd)
    sin = torch.cat([ang.sin(), ang.sin()], -1).to(dtype).view(1, S, 1, hd)
    causal = torch.ones(S, S, dtype=torch.bool).tril()

    def norm(x, w):
        return x * torch.rsqrt((x * x).mean(-1, keepdim=True)
                               + cfg.norm_eps) * w

    def rot(x):
        x1, x2 = x[..., :hd // 2], x[..., hd // 2:]
        return x * cos + torch.cat([-x2, x1], -1) * sin

    with torch.set_grad_enabled(train):
        h = P["embed.weight"][tokens]
        for i in range(cfg.n_layers):
            L = f"layers.{i}."
            qkv = norm(h, P[L + "attn_norm.weight"]) \
                @ P[L + "attn.wqkv.weight"].t()
            q, k, v = qkv.split([Hq * hd, Hkv * hd, Hkv * hd], dim=-1)
            q = rot(q.view(Bt, S, Hq, hd)).transpose(1, 2)
            k = rot(k.view(Bt, S, Hkv, hd)).transpose(1, 2)
            v = v.view(Bt, S, Hkv, hd).transpose(1, 2)
            k = k.repeat_interleave(Hq // Hkv, dim=1)
            v = v.repeat_interleave(Hq // Hkv, dim=1)
            s = (q @ k.transpose(-1, -2)) * hd ** -0.5
            p = torch.softmax(s.masked_fill(~causal, float("-inf")), dim=-1)
            o = (p @ v).transpose(1, 2).reshape(Bt, S, Hq * hd)
            h = h + o @ P[L + "attn.wo.weight"].t()
            gu = norm(h, P[L + "mlp_norm.weight"]) \
                @ P[L + "mlp.w_gate_up.weight"].t()
            I = gu.shape[-1] // 2
            h = h + (F.silu(gu[..., :I]) * gu[..., I:]) \
                @ P[L + "mlp.w_down.weight"].t()
        logits = norm(h, P["norm.weight"]) @ P["lm_head.weight"].t()
        if not train:
            return None, None, logits
        loss = F.cross_entropy(logits.view(Bt * S, -1), targets.view(-1),
                               ignore_index=-100)
        loss.backward()
    return (loss.detach(), {k: p.grad for k, p in P.items()},
            logits.detach())


@functools.lru_cache(maxsize=None)
def _weights(kind):
    """bf16 state dict of the model under test, rounded once. "big": CFG
    with q/k rows of std 0.06 and norm weights 1 + 0.25*randn; "tiny":
    llama_tiny at its default init (what tests/test_model.py runs)."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(0)
        cfg = CFG if kind == "big" else llama_tiny()
        model = Llama(cfg)
        if kind == "big":
            gen = torch.Generator().manual_seed(1)
            nqk = (cfg.n_heads + cfg.n_kv_heads) * cfg.head_dim
            with torch.no_grad():
                for name, p in model.named_parameters():
                    if name.endswith("wqkv.weight"):
                        p[:nqk] = 0.06 * torch.randn(nqk, cfg.dim,
                                                     generator=gen)
                    elif name.endswith("norm.weight"):
                        p.copy_(1 + 0.25 * torch.randn(cfg.dim,
                                                       generator=gen))
    return cfg, {k: v.detach().to(BF16) for k, v in
                 model.state_dict().items()}


@functools.lru_cache(maxsize=None)
def _batch(S, seed, vocab=CFG.vocab_size):
    """(tokens, targets) [B, S] with 37 targets set to -100 (training
    batches; the short inference inputs only use the tokens)."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(0, vocab, (B, S), generator=gen)
    y = torch.randint(0, vocab, (B, S), generator=gen)
    if S >= 130:
        y[0, :7] = -100
        y[1, 100:130] = -100
        assert int((y == -100).sum()) == 37
    return x, y


@functools.lru_cache(maxsize=None)
def _reference(kind, S, seed, dtype, train=True):
    """ref() of one batch, computed once per process and left unchanged."""
    cfg, sd = _weights(kind)
    x, y = _batch(S, seed, cfg.vocab_size)
    return ref(sd, cfg, x, y if train else None, dtype)


def _model(kind, device):
    cfg, sd = _weights(kind)
    with torch.random.fork_rng(devices=[]):
        model = Llama(cfg)
    model = model.to(device=device, dtype=BF16)
    model.load_state_dict(sd)
    return model, cfg


# ---------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------
def _slices(grads, cfg):
    """{name: tensor} with every wqkv gradient cut into its q, k, v rows."""
    hd = cfg.head_dim
    rows = [cfg.n_heads * hd, cfg.n_kv_heads * hd, cfg.n_kv_heads * hd]
    out = {}
    for name, g in grads.items():
        if name.endswith("wqkv.weight"):
            for tag, part in zip("qkv", g.split(rows, dim=0)):
                out[f"{name}[{tag}]"] = part
        else:
            out[name] = g
    return out


def _stats(g, r):
    """(noise, bias) of g against the float64 r."""
    g, r = g.detach().to(F64).cpu(), r.detach().to(F64).cpu()
    d = g - r
    rr = (r * r).sum().item()
    return d.norm().item() / rr ** 0.5, abs((d * r).sum().item() / rr)


def _assert_finite(route, name, t):
    assert bool(torch.isfinite(t.detach().float()).all()), \
        f"{route}: {name}: NaN or inf"


def assert_grad_rule(route, got, ref64, base, cfg, margin=1.0):
    """The noise and bias rules on every gradient slice."""
    got, ref64, base = (_slices(g, cfg) for g in (got, ref64, base))
    assert got.keys() == ref64.keys() == base.keys()
    base_stats = {n: _stats(base[n], ref64[n]) for n in ref64}
    bias_bound = 2 * max(b for _, b in base_stats.values())
    worst_noise = worst_bias = 0.0
    errors = []
    for name, r in ref64.items():
        _assert_finite(route, name, got[name])
        noise, bias = _stats(got[name], r)
        ratio = noise / base_stats[name][0]
        worst_noise = max(worst_noise, ratio)
        worst_bias = max(worst_bias, bias / bias_bound)
        if not ratio <= margin:
            errors.append(
                f"{route}: {name}: noise {noise:.3e} is {ratio:.3f} of the "
                f"naive bf16 baseline's {base_stats[name][0]:.3e} "
                f"(limit {margin})")
        if not bias <= bias_bound:
            errors.append(
                f"{route}: {name}: bias {bias:.3e} is "
                f"{bias / bias_bound:.3f} of the bound {bias_bound:.3e}")
    _note(f"{route}_grad_noise_ratio", worst_noise)
    _note(f"{route}_grad_bias_ratio", worst_bias)
    assert not errors, "\n".join(errors)


def assert_loss_rule(route, loss, loss64, logits64):
    loss = float(loss)
    assert loss == loss and abs(loss) != float("inf"), \
        f"{route}: loss is {loss}"
    bound = 2.0 ** -7 * logits64.abs().max().item()
    err = abs(loss - float(loss64))
    _note(f"{route}_loss_ratio", err / bound)
    assert err <= bound, (f"{route}: loss {loss:.6f} vs float64 "
                          f"{float(loss64):.6f}: error {err:.3e} is "
                          f"{err / bound:.3f} of the bound {bound:.3e}")


def _row_errors(g, r):
    g, r = g.detach().to(F64).cpu(), r.detach().to(F64).cpu()
    return ((g - r).norm(dim=-1) / r.norm(dim=-1)).reshape(-1)


def assert_logits_rule(route, got, ref64, base, rows=None, margin=1.0):
    """got [..., vocab] against the float64 logits ref64 and the naive
    baseline's `base` (both [B, S, vocab]). rows = (batch index, position)
    tensors picks the rows of ref64/base that `got`'s [n, vocab] rows stand
    for; the worst baseline row is taken over the whole input either way.
    The logits are one tensor, so the bias bound's "maximum over all
    slices" is over the two baseline statistics there are: its bias on the
    compared rows and on the whole input (the same thing without `rows`)."""
    _assert_finite(route, "logits", got)
    worst_base_row = _row_errors(base, ref64).max().item()
    bbias = _stats(base, ref64)[1]
    if rows is not None:
        ref64, base = ref64[rows], base[rows]
    assert got.shape == ref64.shape, (route, got.shape, ref64.shape)
    row = _row_errors(got, ref64)
    at = int(row.argmax())
    row_ratio = row[at].item() / worst_base_row
    noise, bias = _stats(got, ref64)
    bnoise, bbias_rows = _stats(base, ref64)
    bbias = max(bbias, bbias_rows)
    _note(f"{route}_logits_row_ratio", row_ratio)
    _note(f"{route}_logits_noise_ratio", noise / bnoise)
    _note(f"{route}_logits_bias_ratio", bias / (2 * bbias))
    assert row_ratio <= margin, (
        f"{route}: logits row {at}: relative L2 error {row[at].item():.3e} "
        f"is {row_ratio:.3f} of the naive bf16 baseline's worst row "
        f"{worst_base_row:.3e} (limit {margin})")
    assert noise <= margin * bnoise, (
        f"{route}: logits: noise {noise:.3e} is {noise / bnoise:.3f} of the "
        f"naive bf16 baseline's {bnoise:.3e} (limit {margin})")
    assert bias <= 2 * bbias, (
        f"{route}: logits: bias {bias:.3e} is {bias / (2 * bbias):.3f} of "
        f"the bound {2 * bbias:.3e}")


def logits_references(state_dict, cfg, tokens):
    """(float64 logits, naive bf16 logits) of ref() for `tokens`: what
    assert_logits_rule wants, for tests that bring their own weights."""
    sd = {k: v.detach().cpu() for k, v in state_dict.items()}
    tokens = tokens.cpu()
    return (ref(sd, cfg, tokens, None, F64)[2],
            ref(sd, cfg, tokens, None, BF16)[2])


# ---------------------------------------------------------------------------
# route spies
# ---------------------------------------------------------------------------
class _CountExt:
    """Passes through to the extension and counts what is asked of it."""

    def __init__(self, ext):
        self._ext = ext
        self.calls = collections.Counter()

    def __getattr__(self, name):
        self.calls[name] += 1
        return getattr(self._ext, name)


class _Spies:
    """impl of every ops.qkv_attention and ops.flash_attention call, the
    number of Attention._sdpa calls and, on the GPU, of every extension
    entry point."""

    def __init__(self, monkeypatch, device):
        self.qkv, self.flash, self.sdpa = [], [], 0
        self.kernels = collections.Counter()
        real_qkv, real_flash = ops.qkv_attention, ops.flash_attention
        real_sdpa = Attention._sdpa

        def qkv_attention(qkv, cos, sin, n_heads, n_kv, impl="ck"):
            self.qkv.append(impl)
            return real_qkv(qkv, cos, sin, n_heads, n_kv, impl)

        def flash_attention(q, k, v, scale=None, impl="ck"):
            self.flash.append(impl)
            return real_flash(q, k, v, scale, impl)

        def _sdpa(attn, *a, **kw):
            self.sdpa += 1
            return real_sdpa(attn, *a, **kw)

        monkeypatch.setattr(ops, "qkv_attention", qkv_attention)
        monkeypatch.setattr(ops, "flash_attention", flash_attention)
        monkeypatch.setattr(Attention, "_sdpa", _sdpa)
        if device == "cuda":
            proxy = _CountExt(ops._ext())
            self.kernels = proxy.calls
            monkeypatch.setattr(ops, "_ext", lambda: proxy)


def _graph_nodes(t):
    """Counter of autograd node type names reachable from t."""
    seen, todo = set(), [t.grad_fn]
    count = collections.Counter()
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        count[type(fn).__name__] += 1
        todo.extend(f for f, _ in fn.next_functions)
    return count


# ---------------------------------------------------------------------------
# training: loss and gradients on every route
# ---------------------------------------------------------------------------
# name -> (S, environment, passes, what the GPU run must have taken)
#   qkv / flash: impl of the ops.qkv_attention / ops.flash_attention calls of
#   one pass; sdpa: Attention._sdpa calls of one pass; nodes: autograd nodes
#   of one loss; kernels: extension entry points of one forward + backward
L = CFG.n_layers
_V3 = dict(qkv=["v3"] * L, flash=[], sdpa=0,
           nodes={"_QKVAttentionBackward": L, "_RopeBackward": 0,
                  "_FlashAttentionBackward": 0},
           kernels={"attn_fwd_v3": L, "attn_grad_pack": L, "attn_bwd_ck": 0})
_SDPA = dict(qkv=[], flash=[], sdpa=L,
             nodes={"_QKVAttentionBackward": 0, "_RopeBackward": 2 * L,
                    "_FlashAttentionBackward": 0},
             kernels={"attn_fwd_v3": 0, "attn_fwd_ck_tr": 0, "attn_fwd": 0,
                      "attn_grad_pack": 0})
TRAIN = {
    "v3": (256, {}, 1, _V3),
    "ck": (384, {}, 1, dict(
        qkv=["ck"] * L, flash=[], sdpa=0,
        nodes={"_QKVAttentionBackward": L, "_RopeBackward": 0},
        kernels={"attn_fwd_ck_tr": L, "attn_fwd_v3": 0,
                 "attn_grad_pack": L})),
    "wmma": (256, {"KT_ATTN": "custom"}, 1, dict(
        qkv=[], flash=["wmma"] * L, sdpa=0,
        nodes={"_QKVAttentionBackward": 0, "_RopeBackward": 2 * L,
               "_FlashAttentionBackward": L},
        kernels={"attn_fwd": L, "attn_fwd_v3": 0, "attn_fwd_ck_tr": 0,
                 "attn_grad_pack": 0})),
    "sdpa": (256, {"KT_ATTN": "torch"}, 1, _SDPA),
    "odd_s": (200, {}, 1, _SDPA),
    "unpacked": (256, {"KT_ATTN_PACK": "0"}, 1, dict(
        qkv=["v3"] * L, flash=["v3"] * L, sdpa=0,
        nodes={"_QKVAttentionBackward": 0, "_RopeBackward": 2 * L,
               "_FlashAttentionBackward": L},
        kernels={"attn_fwd_v3": L, "attn_grad_pack": 0})),
    "ck_backward": (256, {"KT_ATTN_BWD": "ck"}, 1, dict(
        _V3, kernels={"attn_fwd_v3": L, "attn_grad_pack": L,
                      "attn_bwd_ck": L})),
    # the recompute in backward calls the forward a second time
    "checkpointed": (256, {}, 2, dict(
        _V3, kernels={"attn_fwd_v3": 2 * L, "attn_grad_pack": L})),
    "kcontig_off": (256, {"KT_KCONTIG": "0"}, 1, _V3),
    "engine": (256, {}, 1, _V3),
    "accumulate": (256, {}, 1, _V3),
    # ops.WGRAD_LAYOUT lists the 8B shapes only, so at this size every wgrad
    # would take layout "a"; WGRAD_HERE sends each Linear of this model
    # through one of the transposed layouts instead
    "wgrad_layouts": (256, {}, 1, dict(
        _V3, kernels={"attn_fwd_v3": L, "transpose_bf16": 5 * L + 2})),
}
# (in, out) -> layout: wqkv "b", wo and lm_head "d" (both 512 x 512),
# w_gate_up "b", w_down "c": one transpose for "b" and "c", two for "d"
WGRAD_HERE = {(512, 1024): "b", (512, 512): "d", (512, 2048): "b",
              (1024, 512): "c"}
# on the CPU only these two open the gates (as test_model_switch_cpu does);
# every other case falls to Attention._sdpa
CPU_GATED = ("v3", "ck")


def _set_env(monkeypatch, env):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _assert_route(route, device, spies, expect, passes, nodes, micro=1):
    if device == "cpu":
        name = route.split("/")[1]
        if name in CPU_GATED:
            assert spies.qkv == expect["qkv"] * micro and spies.sdpa == 0, \
                f"{route}: took {spies.qkv}, {spies.sdpa} _sdpa calls"
        else:
            assert spies.qkv == [] and spies.sdpa == L * passes * micro, \
                f"{route}: took {spies.qkv}, {spies.sdpa} _sdpa calls"
        return
    assert spies.qkv == expect["qkv"] * passes * micro, (route, spies.qkv)
    assert spies.flash == expect["flash"] * passes * micro, \
        (route, spies.flash)
    assert spies.sdpa == expect["sdpa"] * passes * micro, (route, spies.sdpa)
    for n, want in expect["nodes"].items():
        assert nodes[n] == want, f"{route}: {nodes[n]} {n} nodes, not {want}"
    for n, want in expect["kernels"].items():
        assert spies.kernels[n] == want * micro, \
            f"{route}: {spies.kernels[n]} {n} calls, not {want * micro}"


def _check_model_grads(device, name, monkeypatch):
    S, env, passes, expect = TRAIN[name]
    route = f"{device}/{name}"
    _set_env(monkeypatch, env)
    if device == "cpu" and name in CPU_GATED:
        monkeypatch.setattr(ops, "flash_attention_v3_supported",
                            lambda *a, **kw: name == "v3")
        monkeypatch.setattr(ops, "flash_attention_supported",
                            lambda *a, **kw: True)
    if name == "wgrad_layouts":
        monkeypatch.setattr(ops, "WGRAD_LAYOUT", WGRAD_HERE)
    model, cfg = _model("big", device)
    if name == "checkpointed":
        model.gradient_checkpointing_enable()
    eng = None
    if name == "engine":
        eng = FlatDDP(model, bucket_mb=1)
    elif name == "accumulate":
        eng = FlatDDP(model, bucket_mb=1, grad_accum_steps=2)
    if eng is not None and device == "cuda":
        # dX takes the shadow path only while every shadow is fresh
        linears = [m for m in model.modules() if isinstance(m, ops.Linear)]
        assert linears and all(
            m.weight_t is not None
            and ops.weight_t_is_fresh(m.weight_t, m.weight)
            for m in linears), f"{route}: stale or missing weight_t"
    seeds = (11, 12) if name == "accumulate" else (11,)
    spies = _Spies(monkeypatch, device)
    refs64, bases = [], []
    for seed in seeds:
        x, y = _batch(S, seed)
        loss = model.loss(x.to(device), y.to(device))
        nodes = _graph_nodes(loss)
        loss.backward()
        loss64, g64, logits64 = _reference("big", S, seed, F64)
        assert_loss_rule(route, loss.item(), loss64, logits64)
        refs64.append(g64)
        bases.append(_reference("big", S, seed, BF16)[1])
    if device == "cuda":
        torch.cuda.synchronize()
    if name == "engine":
        got = {n: eng._param_view[p] for n, p in model.named_parameters()}
    else:
        got = {n: p.grad for n, p in model.named_parameters()}
    assert all(g is not None for g in got.values()), route
    got = {n: g.detach().clone() for n, g in got.items()}
    _assert_route(route, device, spies, expect, passes, nodes,
                  micro=len(seeds))
    # two micro-batches: the sum of the two float64 gradients, and the
    # baseline's bf16 sum of its two bf16 gradients
    g64 = {n: sum(r[n] for r in refs64) for n in refs64[0]}
    base = {n: functools.reduce(torch.add, [b[n] for b in bases])
            for n in bases[0]}
    assert_grad_rule(route, got, g64, base, cfg, NOISE_MARGIN[name])


_both("model_grads", _check_model_grads, list(TRAIN))


# ---------------------------------------------------------------------------
# inference: model(tokens) and the KVCache walk
# ---------------------------------------------------------------------------
# prefill of 100, an offset-causal chunk of 60, three single-token steps
KV_CHUNKS = (100, 60, 1, 1, 1)
INFER = ("full_256", "full_200", "kv_cache")


def _check_model_logits(device, name, monkeypatch):
    route = f"{device}/{name}"
    _set_env(monkeypatch, {})
    model, cfg = _model("big", device)
    model.eval()
    spies = _Spies(monkeypatch, device)
    S = sum(KV_CHUNKS) if name == "kv_cache" else int(name.split("_")[1])
    x, _ = _batch(S, 21)
    logits64 = _reference("big", S, 21, F64, False)[2]
    base = _reference("big", S, 21, BF16, False)[2]
    with torch.no_grad():
        if name != "kv_cache":
            got = model(x.to(device))
            if device == "cuda":
                want = (["v3"] * L, 0) if S == 256 else ([], L)
                assert (spies.qkv, spies.sdpa) == want, \
                    (route, spies.qkv, spies.sdpa)
                assert spies.kernels["attn_fwd_v3"] == len(want[0]), route
            assert_logits_rule(route, got, logits64, base,
                               margin=NOISE_MARGIN[name])
            return
        cache = KVCache(cfg, B, 256, torch.device(device), BF16)
        rows, pos = [], 0
        for n in KV_CHUNKS:
            rows.append(model._forward_cached(x[:, pos:pos + n].to(device),
                                              cache))
            pos += n
        assert cache.pos == S and spies.sdpa == L * len(KV_CHUNKS), route
        got = torch.stack(rows, dim=1)                    # [B, chunks, V]
        last = torch.tensor(KV_CHUNKS).cumsum(0) - 1
        picked = (torch.arange(B).view(B, 1).expand(B, len(last)),
                  last.view(1, -1).expand(B, len(last)))
        assert_logits_rule(route, got, logits64, base, rows=picked,
                           margin=NOISE_MARGIN[name])


_both("model_logits", _check_model_logits, list(INFER))


# ---------------------------------------------------------------------------
# the rule must be able to fail
# ---------------------------------------------------------------------------
def _cpu_train(monkeypatch, S=256, seed=11):
    """Loss rule + gradient rule of the CPU model as it stands (patched or
    not) under the default environment."""
    _set_env(monkeypatch, {})
    model, cfg = _model("big", "cpu")
    x, y = _batch(S, seed)
    loss = model.loss(x, y)
    loss.backward()
    loss64, g64, logits64 = _reference("big", S, seed, F64)
    base = _reference("big", S, seed, BF16)[1]
    got = {n: p.grad for n, p in model.named_parameters()}
    assert_grad_rule("mutant", got, g64, base, cfg)
    assert_loss_rule("mutant", loss.item(), loss64, logits64)


def _cpu_tiny_logits(monkeypatch):
    """The logits rule on llama_tiny at its default init: what
    tests/test_model.py asserts of the GPU model."""
    _set_env(monkeypatch, {})
    model, cfg = _model("tiny", "cpu")
    x, _ = _batch(32, 31, cfg.vocab_size)
    with torch.no_grad():
        got = model.eval()(x)
    assert_logits_rule("mutant", got,
                       _reference("tiny", 32, 31, F64, False)[2],
                       _reference("tiny", 32, 31, BF16, False)[2])


def _scaled_backward_rope(factor):
    real = ops._rope_ref

    def rope(x, cos, sin, sign, oscale=1.0):
        out = real(x, cos, sin, sign, oscale)
        return (out.float() * factor).to(out.dtype) if sign < 0 else out
    return rope


def _forward_way_rope():
    real = ops._rope_ref
    return lambda x, cos, sin, sign, oscale=1.0: real(x, cos, sin, 1.0,
                                                      oscale)


def _no_rope():
    real = ops._rope_ref
    return lambda x, cos, sin, sign, oscale=1.0: real(
        x, torch.ones_like(cos), torch.zeros_like(sin), sign, oscale)


def _scaled_rmsnorm_dx():
    real = ops._rmsnorm_ref_bwd

    def bwd(dy, ds, s, w, invrms):
        # only the norm's own dx term: the ds pass-through stays exact
        g, dw = real(dy, None, s, w, invrms)
        g = g.float() * 1.01
        if ds is not None:
            g = g + ds.float().reshape(g.shape)
        return g.to(s.dtype), dw
    return bwd


def _scaled_swiglu(factor):
    real = ops._swiglu_ref_fwd
    return lambda gu: (real(gu).float() * factor).to(gu.dtype)


def _ce_over_numel():
    real = ops.fused_cross_entropy

    def ce(logits, targets, ignore_index=-100):
        # sum / numel == (sum / n_valid) * (n_valid / numel)
        n_valid = int((targets != ignore_index).sum())
        return real(logits, targets, ignore_index) * (n_valid
                                                      / targets.numel())
    return ce


def _add_rmsnorm_without_ds():
    real = ops.add_rmsnorm

    def add_rmsnorm(x, res, w, eps=1e-5):
        y, s = real(x, res, w, eps)
        return y, s.detach()
    return add_rmsnorm


MUTANTS = {
    "rope_backward_x1.01": ("_rope_ref", lambda: _scaled_backward_rope(1.01)),
    "rope_backward_rotates_forward": ("_rope_ref", _forward_way_rope),
    "rmsnorm_dx_x1.01": ("_rmsnorm_ref_bwd", _scaled_rmsnorm_dx),
    "swiglu_x1.01": ("_swiglu_ref_fwd", lambda: _scaled_swiglu(1.01)),
    "ce_divides_by_numel": ("fused_cross_entropy", _ce_over_numel),
    "add_rmsnorm_drops_ds": ("add_rmsnorm", _add_rmsnorm_without_ds),
    "rope_removed": ("_rope_ref", _no_rope),
}
TINY_MUTANTS = {
    "tiny_rope_removed": ("_rope_ref", _no_rope),
    "tiny_swiglu_x1.3": ("_swiglu_ref_fwd", lambda: _scaled_swiglu(1.3)),
}


def test_rule_catches_wrong_models(monkeypatch):
    """The rule passes the CPU model as it is and raises for each of these
    breakages of the reference helpers in ops: on the model above for the
    training rule, and on llama_tiny at its default init for the logits
    rule that tests/test_model.py applies (RoPE removed and SwiGLU x 1.3
    both passed that file's former rtol=5e-2, atol=5e-1)."""
    _cpu_train(monkeypatch)
    _cpu_tiny_logits(monkeypatch)
    for run, mutants in ((_cpu_train, MUTANTS),
                         (_cpu_tiny_logits, TINY_MUTANTS)):
        for name, (attr, make) in mutants.items():
            with monkeypatch.context() as m:
                m.setattr(ops, attr, make())
                with pytest.raises(AssertionError, match="mutant: ") as e:
                    run(m)
                    pytest.fail(f"the rule did not notice {name}",
                                pytrace=False)
                print(f"{name}: {str(e.value).splitlines()[0]}")
