"""Flat-bucket data parallelism for MI355X nodes (RCCL over xGMI).

Design (MI355X-first, not a torch-DDP wrapper):
  * Params are flattened into large contiguous bf16 buckets (default 256 MB)
    — xGMI ring all-reduce is per-link bound (7 links x ~153 GB/s), so fewer,
    larger collectives beat many small ones; 288 GB HBM makes the flat
    copies free.
  * Each param's .grad is a view into its bucket's flat grad buffer, so
    autograd accumulates directly into the comm buffer (zero-copy).
  * A post-accumulate-grad hook counts down per bucket; the moment a bucket
    is complete its all-reduce is launched async on RCCL's comm stream,
    overlapping with the rest of backward.
  * The optimizer is one fused HIP AdamW kernel per bucket (fp32 m/v state,
    bf16 params) — see kubetorch_amd/ops/hip/kernels.hip.

Reference parity: the reference scales jobs, not models —
its DDP is "set RANK/WORLD_SIZE env and let the user call torch DDP"
(reference: serving/spmd/pytorch_process.py:5-41). This module is the
MI355X-native training engine those launchers dispatch.
"""
import os
from typing import List

import torch
import torch.distributed as dist

from kubetorch_amd import ops


def init_distributed(backend=None, timeout_s=300):
    """Initialize torch.distributed from the standard env contract
    (RANK/WORLD_SIZE/LOCAL_RANK/MASTER_ADDR/MASTER_PORT). Returns
    (rank, world_size, local_rank). No-op when WORLD_SIZE<=1."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    if world > 1 and torch.cuda.is_available():
        # RCCL-over-xGMI defaults (also set by the SPMD launcher; this
        # covers direct torchrun launches like the driver's SCALE run):
        # dmabuf-only IPC, no InfiniBand probing intra-node, surfaced
        # comm errors instead of silent hangs
        from kubetorch_amd import constants as _C

        for k, v in _C.RCCL_ENV_DEFAULTS.items():
            os.environ.setdefault(k, v)
    if world > 1 and not dist.is_initialized():
        if backend is None:
            backend = "nccl" if torch.cuda.is_available() else "gloo"
        import datetime

        dist.init_process_group(
            backend=backend, timeout=datetime.timedelta(seconds=timeout_s)
        )
    if torch.cuda.is_available():
        torch.cuda.set_device(local_rank % torch.cuda.device_count())
    return rank, world, local_rank


class _Bucket:
    __slots__ = ("params", "flat_param", "flat_grad", "m", "v", "offsets",
                 "pending", "work", "numel", "completions", "shard_grad",
                 "ema", "flat_param_t", "t_items", "t_table", "t_max_tiles",
                 "t_fallback", "clock")

    def __init__(self):
        self.params: List[torch.nn.Parameter] = []
        self.flat_param = None
        self.flat_grad = None
        self.m = None
        self.v = None
        self.offsets = []
        self.pending = 0
        self.work = None
        self.numel = 0
        self.completions = 0
        # K-contiguous dgrad shadows (FlatDDP._build_shadows)
        self.flat_param_t = None
        self.t_items = []
        self.t_table = None
        self.t_max_tiles = 0
        self.t_fallback = []
        self.clock = None


def _align8(n):
    return (n + 7) & ~7


class FlatDDP:
    """Flat-bucket DP + fused AdamW over a model's parameters.

    Usage:
        engine = FlatDDP(model, lr=3e-4)
        loss = model.loss(x, y); loss.backward(); engine.step()
    """

    def __init__(self, model, lr=3e-4, betas=(0.9, 0.95), eps=1e-8,
                 weight_decay=0.1, bucket_mb=256, process_group=None,
                 overlap_optimizer=True, grad_accum_steps=1, clip_norm=None,
                 zero=False, ema_decay=None, transposed_shadows=None):
        self.model = model
        self.lr = lr
        self.betas = betas
        self.eps = eps
        self.weight_decay = weight_decay
        self.pg = process_group
        self.step_count = 0
        # Global-norm clipping needs the WHOLE grad norm before any param
        # update, so it forces the deferred-optimizer path (bucket
        # all-reduces still overlap backward; only the AdamW launch moves
        # to step()). The clip itself is free: the scale factor rides the
        # fused kernel's grad_scale argument — no extra pass over grads.
        self.clip_norm = clip_norm
        self.last_grad_norm = None
        self._world = (
            dist.get_world_size(process_group) if dist.is_initialized() else 1
        )
        # ZeRO-1: reduce-scatter grads, run AdamW only on this rank's
        # 1/world shard of each bucket (m/v allocated shard-sized), then
        # all-gather the updated params. Cuts optimizer state memory by
        # world (8 GB/B-param -> 1 GB/B-param at 8 GPUs) at the same
        # collective byte count as all-reduce. Deferred-optimizer mode
        # (bucket collectives still overlap backward). NOTE: shards are
        # sized at construction — elastic re-join with a NEW world size
        # needs a fresh engine (load params via load_state_dict).
        self.zero = zero and self._world > 1
        if clip_norm is not None or self.zero:
            overlap_optimizer = False
        # EMA of the weights (fp32, one flat buffer per bucket): updated
        # after every optimizer step; read back via ema_state_dict().
        self.ema_decay = ema_decay
        # Overlap mode: fused AdamW for a bucket is launched on a side HIP
        # stream as soon as the bucket's grads are final (and all-reduced),
        # running concurrently with the remaining backward. Safe because a
        # param's value is only read by its own layer's backward, which has
        # completed by the time its post-accumulate hook fires.
        self._overlap = overlap_optimizer and torch.cuda.is_available()
        self._opt_stream = torch.cuda.Stream() if self._overlap else None
        self._step_started = False
        # copy-mode grads (grad_accum_steps == 1): autograd hands us its
        # freshly-produced grad tensor, the hook copies it into the flat
        # bucket and drops it — no flat-buffer zeroing, no accumulate-add
        # (one full pass over grad bytes saved per step). With accumulation
        # we instead pin .grad to bucket views and zero between optimizer
        # steps.
        self._copy_mode = grad_accum_steps == 1
        self.grad_accum_steps = grad_accum_steps
        # fold mean-over-(ranks x micro-batches) into the fused kernel's
        # grad scale: buckets hold the raw SUM, so the optimizer sees the
        # mean gradient of the effective global batch (no LR surprises
        # when grad_accum_steps changes).
        self._grad_scale = 1.0 / (self._world * grad_accum_steps)
        self._micro_step = 0
        for mod in model.modules():
            if getattr(mod, "ep_world", 1) > 1:
                raise ValueError(
                    "FlatDDP replicates every parameter across the group, "
                    "which would average DIFFERENT experts under expert "
                    "parallelism. Run EP layers with a per-rank optimizer "
                    "(or DP across EP groups) — see models/moe.py.")
        params = [p for p in model.parameters() if p.requires_grad]
        if not params:
            raise ValueError("model has no trainable parameters")
        dtype = params[0].dtype
        dev = params[0].device
        for p in params:
            if p.dtype != dtype:
                raise ValueError("FlatDDP requires uniform param dtype")
        bucket_elems = int(bucket_mb * 1024 * 1024 / dtype.itemsize)

        # Reverse registration order approximates backward completion order,
        # so early buckets finish (and start their all-reduce) first.
        self.buckets: List[_Bucket] = []
        cur = _Bucket()
        for p in reversed(params):
            n = _align8(p.numel())
            if cur.numel + n > bucket_elems and cur.params:
                self.buckets.append(cur)
                cur = _Bucket()
            cur.offsets.append(cur.numel)
            cur.params.append(p)
            cur.numel += n
        self.buckets.append(cur)
        if self.zero:
            # shards must tile the bucket exactly: pad numel to world*8
            align = self._world * 8
            for b in self.buckets:
                b.numel = (b.numel + align - 1) // align * align

        self._param_bucket = {}
        self._param_view = {}
        state_elems = (lambda n: n // self._world) if self.zero else (lambda n: n)
        for b in self.buckets:
            b.flat_param = torch.zeros(b.numel, dtype=dtype, device=dev)
            b.flat_grad = torch.zeros(b.numel, dtype=dtype, device=dev)
            b.m = torch.zeros(state_elems(b.numel), dtype=torch.float32,
                              device=dev)
            b.v = torch.zeros(state_elems(b.numel), dtype=torch.float32,
                              device=dev)
            if self.zero:
                b.shard_grad = torch.zeros(b.numel // self._world,
                                           dtype=dtype, device=dev)
            if self.ema_decay is not None:
                b.ema = None  # lazily initialized from the first params
            for p, off in zip(b.params, b.offsets):
                n = p.numel()
                b.flat_param[off:off + n].copy_(p.data.reshape(-1))
                p.data = b.flat_param[off:off + n].view(p.shape)
                gview = b.flat_grad[off:off + n].view(p.shape)
                if not self._copy_mode:
                    p.grad = gview
                self._param_bucket[p] = b
                self._param_view[p] = gview
                p.register_post_accumulate_grad_hook(self._grad_ready)
            b.pending = len(b.params)
        self._hooks_enabled = True
        # W^T shadows for dgrad: on by default on GPU, forced either way by
        # transposed_shadows (CPU runs take the torch transposes), and off
        # everywhere under KT_KCONTIG=0.
        if transposed_shadows is None:
            transposed_shadows = dev.type == "cuda"
        self.shadows_enabled = bool(transposed_shadows) and \
            ops.kcontig_enabled()
        if self.shadows_enabled:
            self._build_shadows(dtype, dev)
            self.refresh_transposed()

    # -- K-contiguous dgrad shadows -----------------------------------------
    def _build_shadows(self, dtype, dev):
        """One flat W^T buffer per bucket holding an [in, out] copy of every
        ops.Linear weight in it (other params get none), installed on the
        modules as weight_t. The device-side segment table for the one-launch
        refresh is built here, once."""
        mods_of = {}
        for mod in self.model.modules():
            if isinstance(mod, ops.Linear):
                mods_of.setdefault(mod.weight, []).append(mod)
        use_kernel = dev.type == "cuda" and dtype == torch.bfloat16
        for b in self.buckets:
            b.clock = ops.ShadowClock()
            t_numel = 0
            for p, off in zip(b.params, b.offsets):
                if p in mods_of and p.dim() == 2:
                    b.t_items.append((mods_of[p], p, off, t_numel))
                    t_numel += _align8(p.numel())
            if not b.t_items:
                continue
            b.flat_param_t = torch.zeros(t_numel, dtype=dtype, device=dev)
            segs = []
            for item in b.t_items:
                mods, p, off, toff = item
                wt = b.flat_param_t[toff:toff + p.numel()].view(
                    p.shape[1], p.shape[0])
                for mod in mods:
                    mod.weight_t = wt
                if use_kernel and p.shape[0] % 8 == 0 and p.shape[1] % 8 == 0:
                    segs.append((off, toff, p.shape[0], p.shape[1]))
                else:
                    b.t_fallback.append(item)
            if segs:
                b.t_table, b.t_max_tiles = ops.transpose_table(
                    segs, b.flat_param.numel(), t_numel, dev)

    def _touch(self, b):
        """The bucket's params are about to be written: every shadow stamped
        before this no longer counts as fresh."""
        if b.clock is not None:
            b.clock.value = (self.step_count, b.clock.value[1] + 1)

    def _refresh_bucket(self, b):
        """Recompute the bucket's shadows from flat_param on the current
        stream and stamp them fresh."""
        if b.flat_param_t is None:
            return
        if b.t_table is not None:
            ops.transpose_segments_bf16(b.flat_param, b.flat_param_t,
                                        b.t_table, b.t_max_tiles)
        for mods, p, _, _ in b.t_fallback:
            mods[0].weight_t.copy_(p.detach().t())
        for mods, p, _, _ in b.t_items:
            ops.stamp_weight_t(mods[0].weight_t, p, b.clock)

    def mark_params_written(self):
        """Call before writing flat_param from outside the engine; follow
        the write with refresh_transposed()."""
        for b in self.buckets:
            self._touch(b)

    @torch.no_grad()
    def refresh_transposed(self):
        """Rebuild every W^T shadow from the current params. Required after
        any write to flat_param (or to a param in place) that the engine
        did not make itself. Between mark_params_written() (or an in-place
        write through the parameter, which bumps its version) and this
        call, ops.linear sees a stale stamp and uses the plain dY @ W
        path; a raw write to flat_param alone is invisible until here."""
        if not self.shadows_enabled:
            return
        for b in self.buckets:
            self._touch(b)
            self._refresh_bucket(b)

    # -- backward-side -------------------------------------------------------
    def _grad_ready(self, p):
        if not self._hooks_enabled:
            return
        b = self._param_bucket[p]
        view = self._param_view[p]
        if self._copy_mode:
            # autograd allocated this grad; move it into the comm bucket
            # and release it (no accumulate-add, no zeroing pass)
            view.copy_(p.grad.reshape(p.shape))
            p.grad = None
        elif p.grad is not None and p.grad.data_ptr() != view.data_ptr():
            # autograd replaced the view (rare); fold back into the bucket
            view.add_(p.grad)
            p.grad = view
        b.pending -= 1
        if b.pending == 0:
            if self._copy_mode:
                self._bucket_ready(b)
            else:
                # accumulation mode: re-arm per micro-batch; comm + update
                # only once the bucket has seen every micro-batch
                b.pending = len(b.params)
                b.completions += 1
                if b.completions >= self.grad_accum_steps:
                    b.completions = 0
                    self._bucket_ready(b)

    def _bucket_ready(self, b):
        if self._world > 1:
            if self.zero and dist.get_backend(self.pg) == "nccl":
                # true reduce-scatter on RCCL: each rank receives only its
                # 1/world shard (same bytes on the wire as all-reduce)
                b.work = dist.reduce_scatter_tensor(
                    b.shard_grad, b.flat_grad, op=dist.ReduceOp.SUM,
                    group=self.pg, async_op=True)
            else:
                # gloo has no reduce_scatter: all-reduce then slice locally
                # (CPU-CI correctness path)
                b.work = dist.all_reduce(
                    b.flat_grad, op=dist.ReduceOp.SUM, group=self.pg,
                    async_op=True)
        if not self._overlap:
            return
        if not self._step_started:
            self._step_started = True
            self.step_count += 1
        # run this bucket's AdamW on the side stream, ordered after the
        # grad-producing kernels (event) and the all-reduce (work.wait()).
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        with torch.cuda.stream(self._opt_stream):
            self._opt_stream.wait_event(ev)
            if b.work is not None:
                b.work.wait()  # syncs the side stream with the RCCL stream
                b.work = None
            self._touch(b)
            ops.adamw_(
                b.flat_param, b.flat_grad, b.m, b.v, self.lr,
                self.betas[0], self.betas[1], self.eps, self.weight_decay,
                self.step_count, self._grad_scale,
            )
            # same side stream, right behind the update: hidden under the
            # rest of backward like AdamW itself; step() joins the stream
            # before the next forward
            self._refresh_bucket(b)

    # -- optimizer side ------------------------------------------------------
    @torch.no_grad()
    def step(self, lr=None):
        """Finish the update: in overlap mode just join the side stream and
        reset; otherwise wait for all-reduces and run fused AdamW here.
        NOTE (overlap mode): set the LR for step N before its backward."""
        if lr is not None:
            self.lr = lr
        if self._overlap:
            if not self._step_started:  # backward produced no grads
                self.step_count += 1
            torch.cuda.current_stream().wait_stream(self._opt_stream)
            self._step_started = False
        else:
            self.step_count += 1
            grad_scale = self._grad_scale
            for b in self.buckets:
                if b.work is not None:
                    b.work.wait()
                    b.work = None
            if self.zero:
                self._zero_step(grad_scale)
                self._reset_buckets_after_step()
                self._update_ema()
                return
            if self.clip_norm is not None:
                # flat grads hold the SUM over ranks (and micro-batches);
                # the mean grad's norm is ||g_sum|| * grad_scale. Identical
                # on every rank (grads already reduced) — no collective.
                total_sq = sum(
                    (b.flat_grad.float() ** 2).sum() for b in self.buckets
                )
                norm = float(total_sq.sqrt()) * grad_scale
                self.last_grad_norm = norm
                if norm > self.clip_norm:
                    grad_scale *= self.clip_norm / (norm + 1e-6)
            for b in self.buckets:
                self._touch(b)
                ops.adamw_(
                    b.flat_param, b.flat_grad, b.m, b.v, self.lr,
                    self.betas[0], self.betas[1], self.eps, self.weight_decay,
                    self.step_count, grad_scale,
                )
                self._refresh_bucket(b)
        for b in self.buckets:
            if not self._copy_mode:
                b.flat_grad.zero_()
            b.pending = len(b.params)
        self._update_ema()

    def _update_ema(self):
        if self.ema_decay is None:
            return
        d = self.ema_decay
        for b in self.buckets:
            if b.ema is None:
                # copy=True: .float() on fp32 params would ALIAS them
                b.ema = b.flat_param.to(torch.float32, copy=True)
            else:
                b.ema.mul_(d).add_(b.flat_param.float(), alpha=1.0 - d)

    @torch.no_grad()
    def ema_state_dict(self):
        """EMA weights as {param_name: fp32 tensor} (model's names)."""
        if self.ema_decay is None:
            raise ValueError("engine built without ema_decay")
        name_of = {p: n for n, p in self.model.named_parameters()}
        out = {}
        for b in self.buckets:
            ema = b.ema if b.ema is not None else b.flat_param.float()
            for p, off in zip(b.params, b.offsets):
                out[name_of[p]] = ema[off:off + p.numel()].view(p.shape).clone()
        return out

    def _reset_buckets_after_step(self):
        for b in self.buckets:
            if not self._copy_mode:
                b.flat_grad.zero_()
            b.pending = len(b.params)

    def _zero_step(self, grad_scale):
        """ZeRO-1 update: sharded AdamW then all-gather params."""
        world = self._world
        rank = dist.get_rank(self.pg)
        for b in self.buckets:
            sh = b.numel // world
            if dist.get_backend(self.pg) != "nccl":
                b.shard_grad.copy_(b.flat_grad[rank * sh:(rank + 1) * sh])
        if self.clip_norm is not None:
            # each rank holds a disjoint shard of the reduced grads: sum of
            # shard square-norms across ranks = the global square-norm
            total_sq = sum((b.shard_grad.float() ** 2).sum()
                           for b in self.buckets)
            if dist.is_initialized():
                dist.all_reduce(total_sq, op=dist.ReduceOp.SUM, group=self.pg)
            norm = float(total_sq.sqrt()) * grad_scale
            self.last_grad_norm = norm
            if norm > self.clip_norm:
                grad_scale *= self.clip_norm / (norm + 1e-6)
        for b in self.buckets:
            sh = b.numel // world
            shard_param = b.flat_param[rank * sh:(rank + 1) * sh]
            self._touch(b)
            ops.adamw_(
                shard_param, b.shard_grad, b.m, b.v, self.lr,
                self.betas[0], self.betas[1], self.eps, self.weight_decay,
                self.step_count, grad_scale,
            )
            # all-gather the updated shards in place (chunks are views)
            chunks = list(b.flat_param.chunk(world))
            dist.all_gather(chunks, shard_param, group=self.pg)
            self._refresh_bucket(b)

    def zero_grad(self):
        for b in self.buckets:
            if not self._copy_mode:
                b.flat_grad.zero_()
            b.pending = len(b.params)
            b.work = None

    # -- in-step elastic support (parallel/elastic.py) -----------------------
    def abort_comm(self):
        """Forget all in-flight comm state after a collective failure: the
        async works reference a dead process group, and flat grads may hold
        partial sums. The interrupted step is re-run by the caller after
        the group re-forms."""
        for b in self.buckets:
            b.work = None
            b.completions = 0
            b.pending = len(b.params)
            b.flat_grad.zero_()
        self._micro_step = 0
        self._step_started = False
        if self._copy_mode:
            for p in self._param_bucket:
                p.grad = None

    def set_world(self, world):
        """Adopt a new group size after an in-step re-join (zero=False
        only: ZeRO shards are sized by world at construction)."""
        if self.zero:
            raise ValueError("ZeRO-1 engine cannot change world in place")
        self._world = max(1, int(world))
        self._grad_scale = 1.0 / (self._world * self.grad_accum_steps)

    @torch.no_grad()
    def broadcast_params(self, src=0):
        """Sync initial params across ranks (one collective per bucket)."""
        self.mark_params_written()
        if self._world > 1:
            for b in self.buckets:
                dist.broadcast(b.flat_param, src=src, group=self.pg)
        self.refresh_transposed()

    def state_dict(self):
        # NOTE: with zero=True, m/v hold only this rank's shard — resume
        # requires the same world size (save per-rank, or all-gather the
        # state first for a world-size-independent checkpoint).
        return {
            "step": self.step_count,
            "m": [b.m for b in self.buckets],
            "v": [b.v for b in self.buckets],
            "flat_param": [b.flat_param for b in self.buckets],
        }

    def load_state_dict(self, sd):
        self.step_count = sd["step"]
        self.mark_params_written()
        for b, m, v, fp in zip(self.buckets, sd["m"], sd["v"], sd["flat_param"]):
            b.m.copy_(m)
            b.v.copy_(v)
            b.flat_param.copy_(fp)
        self.refresh_transposed()
