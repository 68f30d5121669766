"""Fused clip_grad_norm_ + transformers.AdamW + zero_grad over the engines' flat f32 buffers, and
the linear warm-up schedule (SimANS/co_training/co_training_marco_train.py:57-69, 126-134, 246-254).

One ``step()`` = (optional RCCL all-reduce of the flat gradients) -> global L2 norm (device scalar, no
host sync) -> AdamW update of every tower with the clip coefficient computed on device -> gradients
zeroed in the same pass.  Non-engine parameters (the Reranker's Linear(H,1)) are packed into a small
extra flat buffer so that one code path serves all.
"""
import contextlib
import os

import torch

from . import _lib as L
from .engine import LossScaler

_NO_DECAY = ("bias", "LayerNorm.weight")


def _no_decay(name):
    """The reference's grouping rule (co_training_marco_train.py:59-65): these parameters take no weight decay."""
    return any(k in name for k in _NO_DECAY)


def _saved_state(sd, i):
    """Entry i of a torch Optimizer state_dict's 'state' (the keys are ints, or strings after a trip through JSON), or None."""
    return sd["state"].get(i, sd["state"].get(str(i)))


def _engines_of(model):
    seen, out = set(), []
    for m in model.modules():
        e = getattr(m, "engine", None)
        if e is not None and id(e) not in seen:
            seen.add(id(e))
            out.append((m, e))
    return out


class FusedAdamW(object):
    """AdamW(lr, eps, weight_decay) with the reference's no-decay grouping ('bias', 'LayerNorm.weight')."""

    def __init__(self, model, lr=1e-5, eps=1e-8, weight_decay=0.0, betas=(0.9, 0.999), process_group=None):
        self.model = model
        self.lr, self.eps, self.wd, self.betas = float(lr), float(eps), float(weight_decay), betas
        self.base_lr = float(lr)
        self.step_count = 0
        self.group = process_group
        self.towers = _engines_of(model)
        own = set()
        for m, e in self.towers:
            own.update(id(p) for p in m.parameters())
        self.extra = [p for p in model.parameters() if id(p) not in own and p.requires_grad]
        self.state = {}
        self.param_groups = [{"lr": self.lr}]           # scheduler-facing view
        self._sq = None
        # fp16 towers: this optimiser's dynamic loss scale (amp.initialize(model, optimizer, opt_level='O1') creates one
        # scaler per optimizer too, co_training_marco_train.py:97-104); engines read it in backward, step() updates it
        self.scaler = None
        if any(e.dtype_code == L.SIMX_F16 for m, e in self.towers):
            self.scaler = LossScaler(init_scale=float(os.environ.get("SIMX_LOSS_SCALE_INIT", 2.0 ** 16)))
            for m, e in self.towers:
                if e.dtype_code == L.SIMX_F16:
                    e.scaler = self.scaler
        # data parallelism (enable_overlap): gradient slices are all-reduced on a side stream as soon as the backward
        # has finished them; step() only waits for what is still in flight
        self.world_size = 1
        self.armed = True                                # False while accumulating micro-steps (no reduction yet)
        self.payload = "fp32"                            # "bf16": gradient slices cross the links as bf16 (half the bytes)
        self.profile_comm = False                        # bench.py --gpus N: per-step communication timings (comm_stats())
        self._comm = None
        self._hooks_on = False
        self._pending = []                               # [(work, engine, lo, hi, payload buffer or None, events or None)]
        self._reduced = {}                               # id(engine) -> backward serial whose slices were launched
        self._synced = False
        self._comm_log = []

    def _device(self):
        """Where the flat buffers live: the towers' device, without towers the extra parameters'."""
        return self.towers[0][1].flat.device if self.towers else self.extra[0].device

    def _on_gpu(self):
        return bool(self.towers) and self._device().type == "cuda"

    def _join_tower_streams(self, cur):
        """A tower's backward may have run on a side stream (BiBertEncoder): nothing queued on `cur` reads its buffers before."""
        for m, e in self.towers:
            st = getattr(e, "last_stream", None)
            if st is not None and st != cur:
                cur.wait_stream(st)

    def _comm_ctx(self):
        """-> (the communication stream, None on the host; the context that makes it the current stream)"""
        comm = self._comm if self._on_gpu() else None
        return comm, (torch.cuda.stream(comm) if comm is not None else contextlib.nullcontext())

    # ---- DDP's role: gradient averaging over the ranks (co_training_marco_train.py:107-114) ------------------------
    def enable_overlap(self, world_size, parts=2, process_group=None, payload=None, force=False):
        """One process per GPU, RCCL: every tower's backward runs in `parts` layer ranges (simx_bert_bwd_range) and each
        finished slice of the flat gradient buffer is all-reduced asynchronously on a communication stream while the
        remaining layers -- and the other tower -- are still in backward.  The query tower's reduction hides under the
        passage tower's backward, the upper half of the passage tower's under its lower half.  With gradient accumulation
        set ``armed = False`` for all but the last micro-step: an in-place accumulated buffer must be reduced ONCE, and a
        backward into a buffer whose slices are already on the wire raises (see _on_grad_ready).  `payload="bf16"` sends
        the slices as bf16 (half the bytes; the sum is taken in bf16 by RCCL, the master copy stays f32).
        `force`: install the hooks for a one-rank group as well (the RCCL smoke test of the whole path on one GPU)."""
        self.world_size = int(world_size)
        if process_group is not None:
            self.group = process_group
        if payload is None:
            # default: the payload follows the engine's arithmetic.  f32 engines (every shipped recipe; the mode held to
            # north_star's 1e-3) all-reduce f32 like the reference's DDP (co_training_marco_train.py:107-114); only when EVERY
            # tower computes in 16 bits do the slices cross the links as bf16 (438 MB instead of 876 MB per step and
            # rank; the sum is taken in bf16 by RCCL, the master gradients stay f32).  SIMX_GRAD_PAYLOAD=bf16|fp32 overrides.
            all16 = bool(self.towers) and all(getattr(e, "dtype_code", None) in (L.SIMX_BF16, L.SIMX_F16) for _, e in self.towers)
            payload = os.environ.get("SIMX_GRAD_PAYLOAD") or ("bf16" if self.world_size > 1 and all16 else "fp32")
        if payload not in ("fp32", "bf16"):
            raise ValueError("payload must be 'fp32' or 'bf16', got %r" % (payload,))
        self.payload = payload
        if self.world_size <= 1 and not force:
            return self
        self._comm = torch.cuda.Stream(device=self._device()) if self._on_gpu() else None
        self._hooks_on = True
        for m, e in self.towers:
            e.grad_ready_hook = self._on_grad_ready
            e.bwd_parts = parts
        return self

    def _on_grad_ready(self, e, lo, hi):
        if not self.armed or not self._hooks_on or hi <= lo:
            return
        import torch.distributed as dist
        self._reduced[id(e)] = e._bwd_serial
        e._reduced_this_step = True                      # a further backward into this buffer before step() raises
        sl = e.flat_grad[lo:hi]
        ev, ctx = None, contextlib.nullcontext()         # (host tensors: the gloo control-flow tests)
        if e.flat_grad.is_cuda:
            cur = torch.cuda.current_stream()
            comm = self._comm or cur
            comm.wait_stream(cur)                        # the slice is final once the backward kernels queued so far are done
            ctx = torch.cuda.stream(comm)
            if self.profile_comm:
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        with ctx:
            if ev is not None:
                ev[0].record(comm)
            buf = sl.to(torch.bfloat16) if self.payload == "bf16" else None
            w = dist.all_reduce(buf if buf is not None else sl, op=dist.ReduceOp.SUM, group=self.group, async_op=True)
        self._pending.append((w, e, lo, hi, buf, ev))

    def sync_grads(self, world_size=None):
        """Completes the gradient reduction of this step (idempotent until the next step()): joins the streams the towers'
        backward ran on, waits for the slices launched by the backward hooks, reduces whatever was not launched (no hooks,
        un-armed micro-steps, the small non-engine parameters) synchronously.  -> the factor that turns the summed
        gradients into the DDP mean (1/W)."""
        W = int(world_size if world_size is not None else self.world_size)
        if W <= 1 and not self._hooks_on:
            return 1.0
        if self._synced:
            return 1.0 / W
        import torch.distributed as dist
        cur = torch.cuda.current_stream() if self._on_gpu() else None
        if cur is not None:
            self._join_tower_streams(cur)
        launched = set()
        nbytes, evs = 0, []
        comm, ctx = self._comm_ctx()
        with ctx:
            for w, e, lo, hi, buf, ev in self._pending:
                w.wait()                                  # RCCL: the communication stream waits for the collective, not the host
                if buf is not None:
                    e.flat_grad[lo:hi].copy_(buf)
                if ev is not None:
                    ev[1].record(comm)
                    evs.append(ev)
                launched.add(id(e))
                nbytes += (hi - lo) * (2 if buf is not None else 4)
        self._pending = []
        t_wait = None
        if comm is not None:
            if self.profile_comm:
                t_wait = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                t_wait[0].record(cur)
            cur.wait_stream(comm)
            if t_wait is not None:
                t_wait[1].record(cur)
        for m, e in self.towers:
            if id(e) not in launched:
                g = e.ensure_grad()
                if self.payload == "bf16":
                    b = g.to(torch.bfloat16)
                    dist.all_reduce(b, op=dist.ReduceOp.SUM, group=self.group)
                    g.copy_(b)
                else:
                    dist.all_reduce(g, op=dist.ReduceOp.SUM, group=self.group)
                nbytes += g.numel() * (2 if self.payload == "bf16" else 4)
            e._open_graphs = 0
        if self.extra:
            st = self._extra_state(self._device())
            self._gather_extra(st)
            dist.all_reduce(st["g"], op=dist.ReduceOp.SUM, group=self.group)
            st["g_ready"] = True
            nbytes += st["g"].numel() * 4
        if self.profile_comm:
            self._comm_log.append((nbytes, evs, t_wait, len(launched)))
        self._synced = True
        return 1.0 / W

    def comm_stats(self):
        """Per-step communication figures collected while ``profile_comm`` was on (synchronises): bytes this rank put on the
        wire, milliseconds the all-reduces occupied the communication stream, milliseconds the compute stream had to wait
        for them in step() (the exposed part), slices launched from the backward hooks."""
        if not self._comm_log:
            return None
        torch.cuda.synchronize()
        n = len(self._comm_log)
        tot_b = sum(b for b, _, _, _ in self._comm_log)
        ar = sum(sum(a.elapsed_time(b) for a, b in evs) for _, evs, _, _ in self._comm_log)
        ex = sum(t[0].elapsed_time(t[1]) for _, _, t, _ in self._comm_log if t is not None)
        return {"steps": n, "allreduce_bytes_per_step": tot_b // n, "payload": self.payload,
                "allreduce_ms_on_comm_stream_per_step": round(ar / n, 3), "exposed_wait_ms_per_step": round(ex / n, 3),
                "overlapped_slices_per_step": sum(k for _, evs, _, k in self._comm_log) / float(n)}

    def _extra_slices(self):
        """(index, parameter, element offset, elements) of every extra parameter in the packed buffer."""
        o = 0
        for j, p in enumerate(self.extra):
            yield j, p, o, p.numel()
            o += p.numel()

    def _gather_extra(self, st):
        for j, p, o, n in self._extra_slices():
            st["p"][o:o + n].copy_(p.reshape(-1))
            if p.grad is not None:
                st["g"][o:o + n].copy_(p.grad.reshape(-1))

    def _tower_state(self, e):
        st = self.state.get(id(e))
        if st is None or st["m"].device != e.flat.device:
            st = {"m": torch.zeros_like(e.flat), "v": torch.zeros_like(e.flat)}
            self.state[id(e)] = st
        return st

    def _extra_state(self, dev):
        st = self.state.get("extra")
        n = sum(p.numel() for p in self.extra)
        if st is None or st["p"].device != dev:
            pad = (n + 3) // 4 * 4
            st = {k: torch.zeros(pad, dtype=torch.float32, device=dev) for k in ("p", "g", "m", "v")}
            st["n"] = n
            st["g_ready"] = False
            self.state["extra"] = st
        return st

    def _discard_pending(self):
        """Drop a step whose gradient reduction is already on the wire (zero_grad() without step(), e.g. after a non-finite
        loss): the collectives launched by the backward hooks are waited for on the communication stream, the compute stream
        joins it -- nothing may zero a buffer RCCL is still reading or writing -- and the per-step bookkeeping is reset so
        that the next backward may arm its slices again."""
        if self._pending:
            comm, ctx = self._comm_ctx()
            with ctx:
                for w, e, lo, hi, buf, ev in self._pending:
                    w.wait()
            if comm is not None:
                torch.cuda.current_stream().wait_stream(comm)
            self._pending = []
        self._reduced = {}
        self._synced = False
        for m, e in self.towers:
            e._reduced_this_step = False
        st = self.state.get("extra")
        if st is not None:
            st["g_ready"] = False

    def zero_grad(self, set_to_none=False):
        self._discard_pending()
        for m, e in self.towers:
            if e.flat_grad is not None:
                e.flat_grad.zero_()
            e._open_graphs = 0                         # forwards that never got a backward no longer hold the hooks back
        for p in self.extra:
            if p.grad is not None:
                p.grad.zero_()

    @torch.no_grad()
    def step(self, max_grad_norm=0.0, world_size=1):
        """Returns the device scalar holding the squared global grad norm (before clipping)."""
        lr = self.param_groups[0]["lr"]
        self.step_count += 1
        bufs, sq, clip, grad_scale, sc = self._prepare(max_grad_norm, world_size)
        self._apply(bufs, lr, sq if clip else None, float(max_grad_norm or 0.0), grad_scale, sc)
        self._sq = sq
        return sq

    def _prepare(self, max_grad_norm, world_size):
        """Everything of a step that is not the update rule: joins the towers' streams, completes the gradient reduction,
        collects the flat buffers, takes the deterministic squared norm and lets the loss scaler judge it.
        -> ([(p, g, state, engine or None)], squared norm, clip?, 1/W, scaler state or None)"""
        dev = self._device()
        self._join_tower_streams(torch.cuda.current_stream())
        s = L.stream_ptr()
        grad_scale = self.sync_grads(max(int(world_size), self.world_size))
        self._synced = False
        self._reduced = {}
        bufs = []
        for m, e in self.towers:
            bufs.append((e.flat, e.ensure_grad(), self._tower_state(e), e))
            e._open_graphs = 0
            e._reduced_this_step = False
        if self.extra:
            st = self._extra_state(dev)
            if not st.get("g_ready"):
                self._gather_extra(st)
            st["g_ready"] = False
            bufs.append((st["p"], st["g"], st, None))
        sq = torch.zeros(1, dtype=torch.float32, device=dev)
        clip = bool(max_grad_norm and max_grad_norm > 0)
        if clip or self.scaler is not None:       # (the fp16 overflow check is the same norm: inf / nan in any gradient)
            ws = torch.empty(L.SIMX_SQNORM_WS_FLOATS, dtype=torch.float32, device=dev)
            for p_, g_, st_, e_ in bufs:          # (no float atomics: every data-parallel replica gets the same bits)
                L.call("simx_sqnorm_accum_det", s, L.ptr(g_), g_.numel(), L.ptr(sq), L.ptr(ws))
        sc = None
        if self.scaler is not None:
            self.scaler.update(sq)                # device side: skip + halve on overflow, count, grow
            sc = self.scaler.state(dev)
        return bufs, sq, clip, grad_scale, sc

    def _apply(self, bufs, lr, sq, max_norm, grad_scale, sc):
        """The update rule over the prepared buffers (`sq`: None when the step does not clip)."""
        s = L.stream_ptr()
        for p_, g_, st_, e_ in bufs:
            L.call("simx_adamw_step_sc", s, L.ptr(p_), L.ptr(g_), L.ptr(st_["m"]), L.ptr(st_["v"]), p_.numel(), lr,
                   self.betas[0], self.betas[1], self.eps, 0.0, self.step_count,
                   L.ptr(sq), max_norm, grad_scale, 1, L.ptr(sc))
            if e_ is not None:
                e_.mark_weights_dirty()
        # decoupled decay p -= lr*wd*p on everything except 'bias' / 'LayerNorm.weight' (co_training_marco_train.py:59-65; default
        # weight_decay is 0.0); on an overflow-skipped fp16 step the factor is 1: the device flag, no host read
        keep = None if sc is None else 1.0 - sc[3]
        f = 1.0 - lr * self.wd * (1.0 if keep is None else keep) if self.wd > 0.0 or self.extra else None
        if self.wd > 0.0:
            self._decay_towers(f)
        if self.extra:
            names = {id(p): n for n, p in self.model.named_parameters()}

            def decay(p):
                if self.wd > 0.0 and not _no_decay(names[id(p)]):
                    p.mul_(f)
            self._scatter_extra(decay)

    def _scatter_extra(self, after=None):
        """The packed extra parameters back into their tensors (`after(p)`: what the update still owes each), gradients zeroed."""
        st = self.state["extra"]
        for j, p, o, n in self._extra_slices():
            p.copy_(st["p"][o:o + n].view_as(p))
            if after is not None:
                after(p)
            if p.grad is not None:
                p.grad.zero_()

    def _decay_towers(self, f):
        for m, e in self.towers:
            for name, p in m.named_parameters():
                if not _no_decay(name):
                    p.mul_(f)
            e.mark_weights_dirty()

    # ---- state interchange with the reference's checkpoints (co_training_marco_train.py:310-358) ------------------------
    def _ref_param_order(self):
        """The reference builds transformers.AdamW from two groups in named_parameters() order -- decayed parameters first,
        then the 'bias' / 'LayerNorm.weight' ones (co_training_marco_train.py:57-65) -- and torch numbers optimizer state by
        position in that concatenation.  -> [(name, param, group)]"""
        named = list(self.model.named_parameters())
        return [(n, p, 0) for n, p in named if not _no_decay(n)] + [(n, p, 1) for n, p in named if _no_decay(n)]

    def _moment_views(self):
        """{id(param): (m_view, v_view)} into the flat Adam-state buffers."""
        out = {}
        for m, e in self.towers:
            st = self._tower_state(e)
            mv, vv = e.views(st["m"]), e.views(st["v"])
            for name, p in m.named_parameters():
                out[id(p)] = (mv[name], vv[name])
        if self.extra:
            st = self._extra_state(self._device())
            for j, p, o, n in self._extra_slices():
                out[id(p)] = (st["m"][o:o + n].view_as(p), st["v"][o:o + n].view_as(p))
        return out

    _group_defaults = {"correct_bias": True}         # what the reference's optimizer class adds to every param group

    def _state_extras(self):
        """None: every parameter has a state entry of step / exp_avg / exp_avg_sq.  A subclass returns {id(param): further
        entries} for the parameters that have stepped; the others get no entry."""
        return None

    def state_dict(self):
        """torch.optim.Optimizer.state_dict() of the reference's transformers.AdamW: {'state': {i: {'step', 'exp_avg',
        'exp_avg_sq'}}, 'param_groups': [decay group, no-decay group]} -- a checkpoint written here resumes in the reference
        and the other way round."""
        order = self._ref_param_order()
        views = self._moment_views()
        state = {}
        # (fp16: steps the scaler skipped did not age the moments -- apex skips optimizer.step() on them as well)
        applied = self.step_count if self.scaler is None else self.scaler.snapshot()["applied_steps"]
        if applied > 0:
            more = self._state_extras()
            for i, (n, p, g) in enumerate(order):
                if more is not None and id(p) not in more:
                    continue
                mv, vv = views[id(p)]
                state[i] = {"step": applied, "exp_avg": mv.detach().cpu().clone(), "exp_avg_sq": vv.detach().cpu().clone()}
                if more is not None:
                    state[i].update(more[id(p)])
        lr = self.param_groups[0]["lr"]
        base = dict(lr=lr, initial_lr=self.base_lr, betas=tuple(self.betas), eps=self.eps, **self._group_defaults)
        n0 = sum(1 for _, _, g in order if g == 0)
        out = {"state": state,
               "param_groups": [dict(base, weight_decay=self.wd, params=list(range(n0))),
                                dict(base, weight_decay=0.0, params=list(range(n0, len(order))))]}
        if self.scaler is not None:
            out["loss_scaler"] = self.scaler.state_dict()     # (extra key: torch's Optimizer.load_state_dict ignores it)
        return out

    def load_state_dict(self, sd):
        if "towers" in sd:                              # round-1 format of this package (flat buffers)
            self.step_count = sd["step"]
            self.param_groups[0]["lr"] = sd.get("lr", self.lr)
            for (m, e), t in zip(self.towers, sd["towers"]):
                st = self._tower_state(e)
                st["m"].copy_(t["m"])
                st["v"].copy_(t["v"])
            if "extra" in sd and self.extra:
                st = self._extra_state(self._device())
                for k in ("p", "g", "m", "v"):
                    st[k].copy_(sd["extra"][k])
            return
        if "state" not in sd or "param_groups" not in sd:
            raise ValueError("optimizer state is neither a torch Optimizer state_dict nor this package's flat format: keys %s"
                             % sorted(sd.keys()))
        order = self._ref_param_order()
        n_saved = sum(len(g["params"]) for g in sd["param_groups"])
        if n_saved != len(order):
            raise ValueError("optimizer state has %d parameters, this model has %d (different architecture or share_weight)"
                             % (n_saved, len(order)))
        views = self._moment_views()
        steps = set()
        with torch.no_grad():
            for i, (n, p, g) in enumerate(order):
                st = _saved_state(sd, i)
                if st is None:
                    continue
                if tuple(st["exp_avg"].shape) != tuple(p.shape):
                    raise ValueError("optimizer state %d (%s): shape %s vs parameter %s" % (i, n, tuple(st["exp_avg"].shape), tuple(p.shape)))
                mv, vv = views[id(p)]
                mv.copy_(st["exp_avg"].to(torch.float32))
                vv.copy_(st["exp_avg_sq"].to(torch.float32))
                steps.add(int(st["step"]))
        if len(steps) > 1:
            raise ValueError("per-parameter step counts differ (%s): the fused update keeps one step count" % sorted(steps))
        self.step_count = steps.pop() if steps else 0
        if self.scaler is not None:
            ls = dict(sd.get("loss_scaler") or {"scale": self.scaler.init_scale})
            ls["applied_steps"] = self.step_count
            self.scaler.load_state_dict(ls, self._device())
        g0 = sd["param_groups"][0]
        self.param_groups[0]["lr"] = float(g0.get("lr", self.lr))
        self.base_lr = float(g0.get("initial_lr", self.base_lr))


_LAMB_CHUNK_T = [("seg", "<i4"), ("len", "<i4"), ("off", "<i8")]      # simx_lamb_chunk_t (include/simx.h)
_LAMB_SCALARS = ("weight_norm", "adam_norm", "trust_ratio")


def lamb_chunk_plan(segs, chunk):
    """The host side of simx_lamb_step's plan.  `segs`: [(offset, elements, weight decay)] ascending and disjoint.
    -> (chunks [simx_lamb_chunk_t], seg_chunks int32 [nseg, 2], seg_range int64 [nseg, 2], seg_wd f32 [nseg]) as NumPy arrays:
    every segment is cut into chunks of `chunk` elements and a ragged last one, so no chunk crosses a segment."""
    import numpy as np
    parts, seg_chunks, at = [], np.zeros((len(segs), 2), np.int32), 0
    for i, (off, n, wd) in enumerate(segs):
        k = (n + chunk - 1) // chunk
        c = np.zeros(k, dtype=_LAMB_CHUNK_T)
        start = np.arange(k, dtype=np.int64) * chunk
        c["seg"], c["off"], c["len"] = i, off + start, np.minimum(chunk, n - start)
        parts.append(c)
        seg_chunks[i] = (at, k)
        at += k
    chunks = np.concatenate(parts) if parts else np.zeros(0, dtype=_LAMB_CHUNK_T)
    seg_range = np.array([(off, n) for off, n, wd in segs], dtype=np.int64).reshape(len(segs), 2)
    return chunks, seg_chunks, seg_range, np.array([wd for off, n, wd in segs], dtype=np.float32)


class FusedLamb(FusedAdamW):
    """Lamb(lr, eps, weight_decay) of PROD/ProD_KD/utils/lamb.py (get_optimizer's --optimizer lamb; no bias correction, trust
    ratio min(|p|, 10) / |u| per parameter tensor) with the reference's no-decay grouping.  Everything that is not the update
    rule -- towers, the extra-parameter buffer, gradient reduction, loss scaler, norm, schedule view -- is FusedAdamW's.

    One parameter = one HF tensor = one segment of simx_lamb_step's plan: an entry of the engine's layout (the fused QKV slots
    are three segments each), or one packed extra parameter.  The reference skips parameters whose gradient is None; here
    that is a tower's pooler.dense.* (never computed) and any extra parameter without a gradient: they are in no segment and
    keep their bits, also under weight decay."""

    _group_defaults = {}

    def __init__(self, model, lr=1e-3, eps=1e-6, weight_decay=0.0, betas=(0.9, 0.999), process_group=None):
        super(FusedLamb, self).__init__(model, lr=lr, eps=eps, weight_decay=weight_decay, betas=betas, process_group=process_group)
        self._plan = None
        self._carry = {}        # id(param) -> (weight_norm, adam_norm, trust_ratio) waiting for a plan that holds the parameter

    # ---- the segment table ---------------------------------------------------------------------------------------------
    def segments(self, live_extra=None):
        """[(name in the model, buffer, element offset, elements, weight decay, parameter)] by buffer, ascending in offset
        within each (the plan's order; engine.layout is in HF registration order, where a layer's query bias comes between
        its query and key weights while the flat buffer holds the three weights back to back): buffer i < number of towers is
        tower i's flat buffer, the last one the packed extra parameters (`live_extra`: one flag per extra parameter, False
        leaves it out; None takes all)."""
        names = {}
        for n, p in self.model.named_parameters():
            names.setdefault(id(p), n)
        wd = lambda n: 0.0 if _no_decay(n) else self.wd
        out = []
        for b, (m, e) in enumerate(self.towers):
            own = dict(m.named_parameters())
            for key, off, shape in sorted(e.layout, key=lambda entry: entry[1]):
                if key.startswith("pooler.") or key not in own:
                    continue
                p = own[key]
                out.append((names[id(p)], b, int(off), p.numel(), wd(names[id(p)]), p))
        for j, p, o, n in self._extra_slices():
            if live_extra is None or live_extra[j]:
                out.append((names[id(p)], len(self.towers), o, n, wd(names[id(p)]), p))
        return out

    def _plan_for(self, dev):
        """The plan tables of every buffer on `dev`, built once (again only when the device, or the set of extra parameters
        that carry a gradient, changes) and checked on the host by simx_lamb_plan_check before they are uploaded.  All
        segments' stats rows live in ONE device tensor (NaN = not computed yet), so trust_ratios() is one copy."""
        import numpy as np
        live = tuple(p.grad is not None for p in self.extra)
        key = (str(dev), live)
        if self._plan is not None and self._plan["key"] == key:
            return self._plan
        if self._plan is not None:                       # rows computed so far follow their parameters into the new plan
            self._carry.update(self._stats_rows())
        lib = L.load()
        chunk = int(lib.simx_lamb_chunk())
        segs = self.segments(live)
        sizes = [e.flat.numel() for m, e in self.towers] + ([self._extra_state(dev)["p"].numel()] if self.extra else [])
        stats = np.full((len(segs), 3), np.nan, dtype=np.float32)
        for i, sg in enumerate(segs):
            if id(sg[5]) in self._carry:
                stats[i] = self._carry.pop(id(sg[5]))
        dstats = torch.from_numpy(stats).to(dev)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)
        bufs, row, most = [], 0, 1
        for b, n in enumerate(sizes):
            mine = [sg for sg in segs if sg[1] == b]
            if not mine:
                bufs.append(None)
                continue
            chunks, seg_chunks, seg_range, seg_wd = lamb_chunk_plan([(sg[2], sg[3], sg[4]) for sg in mine], chunk)
            hp = lambda a: a.ctypes.data_as(L.C.c_void_p)
            L.call("simx_lamb_plan_check", hp(chunks), len(chunks), hp(seg_chunks), hp(seg_range), len(mine), n)
            bufs.append({"chunks": up(chunks), "nchunk": len(chunks), "seg_chunks": up(seg_chunks), "seg_wd": up(seg_wd),
                         "nseg": len(mine), "stats": dstats[row:row + len(mine)]})
            row += len(mine)
            most = max(most, len(chunks))
        self._plan = {"key": key, "segs": segs, "bufs": bufs, "stats": dstats,
                      "partials": torch.empty(2 * most, dtype=torch.float32, device=dev)}
        return self._plan

    def _stats_rows(self):
        """{id(param): (weight_norm, adam_norm, trust_ratio)} of the current plan: one device-to-host copy."""
        if self._plan is None:
            return {}
        rows = self._plan["stats"].cpu().numpy()
        return {id(sg[5]): tuple(float(x) for x in rows[i]) for i, sg in enumerate(self._plan["segs"])}

    def trust_ratios(self):
        """{parameter name: (weight_norm, adam_norm, trust_ratio)} of the last applied step, for every parameter that steps
        (what the reference's log_lamb_rs puts into its histograms).  One device-to-host copy."""
        rows = self._stats_rows()
        return {sg[0]: rows[id(sg[5])] for sg in (self._plan["segs"] if self._plan is not None else [])}

    # ---- the update rule -----------------------------------------------------------------------------------------------
    def _apply(self, bufs, lr, sq, max_norm, grad_scale, sc):
        plan = self._plan_for(bufs[0][0].device)
        s = L.stream_ptr()
        for (p_, g_, st_, e_), b in zip(bufs, plan["bufs"]):
            if b is None:
                continue
            L.call("simx_lamb_step", s, L.ptr(p_), L.ptr(g_), L.ptr(st_["m"]), L.ptr(st_["v"]), p_.numel(), L.ptr(b["chunks"]),
                   b["nchunk"], L.ptr(b["seg_chunks"]), L.ptr(b["seg_wd"]), b["nseg"], L.ptr(b["stats"]), L.ptr(plan["partials"]),
                   lr, self.betas[0], self.betas[1], self.eps, L.ptr(sq), max_norm, grad_scale, 1, L.ptr(sc))
            if e_ is not None:
                e_.mark_weights_dirty()
        if self.extra:
            self._scatter_extra()                        # (the decay is inside u)

    # ---- state interchange: torch.optim.Optimizer.state_dict() of the reference's Lamb ----------------------------------
    def _state_extras(self):
        """Parameters in a segment (or still waiting for one after a load) have stepped; the three scalars appear once they
        have been computed or loaded (an AdamW-shaped state carries none: the next step computes them)."""
        rows = dict(self._carry)
        rows.update(self._stats_rows())
        out = {}
        for pid, row in rows.items():
            out[pid] = {} if any(x != x for x in row) else {k: torch.tensor(x, dtype=torch.float32) for k, x in zip(_LAMB_SCALARS, row)}
        return out

    def load_state_dict(self, sd):
        """Reads the reference's Lamb layout and, moments only, transformers.AdamW's (and FusedAdamW's formats)."""
        super(FusedLamb, self).load_state_dict(sd)
        if "state" not in sd:
            return
        nan = float("nan")
        self._plan, self._carry = None, {}
        stepping = {id(sg[5]) for sg in self.segments()}       # (an AdamW state has entries for the pooler slots as well)
        for i, (n, p, g) in enumerate(self._ref_param_order()):
            st = _saved_state(sd, i)
            if st is not None and id(p) in stepping:
                self._carry[id(p)] = tuple(float(st[k]) if k in st else nan for k in _LAMB_SCALARS)


class LinearWarmupSchedule(object):
    """get_linear_schedule_with_warmup (co_training_marco_train.py:126-134): lr*t/warm, then linear to 0."""

    def __init__(self, optimizer, num_warmup_steps, num_training_steps, last_step=0):
        self.opt, self.warm, self.total = optimizer, float(num_warmup_steps), float(num_training_steps)
        self.base = optimizer.base_lr
        self.t = last_step
        self._apply()

    def factor(self, t):
        if t < self.warm:
            return float(t) / float(max(1.0, self.warm))
        return max(0.0, float(self.total - t) / float(max(1.0, self.total - self.warm)))

    def _apply(self):
        self.opt.param_groups[0]["lr"] = self.base * self.factor(self.t)

    def step(self):
        self.t += 1
        self._apply()

    def get_last_lr(self):
        return [self.opt.param_groups[0]["lr"]]

    def state_dict(self):
        """torch LambdaLR.state_dict() (what the reference checkpoints as scheduler_dict; lr_lambdas holds None for a plain
        function) -- last_epoch is the number of scheduler.step() calls."""
        return {"base_lrs": [self.base], "last_epoch": int(self.t), "_step_count": int(self.t) + 1, "verbose": False,
                "_get_lr_called_within_step": False, "_last_lr": self.get_last_lr(), "lr_lambdas": [None],
                "num_warmup_steps": self.warm, "num_training_steps": self.total}

    def load_state_dict(self, sd):
        if "last_epoch" in sd:                          # torch LambdaLR (the reference) or this class
            self.t = int(sd["last_epoch"])
            if sd.get("base_lrs"):
                self.base = float(sd["base_lrs"][0])
            self.warm = float(sd.get("num_warmup_steps", self.warm))       # (a LambdaLR dict does not carry the schedule shape:
            self.total = float(sd.get("num_training_steps", self.total))   #  it stays what the constructor was given)
        elif "t" in sd:                                 # round-1 format: written when the train loop still called
            # scheduler.step() BEFORE optimizer.step(), i.e. `t` had already been advanced for the update it was saved after;
            # under today's order (optimizer first, as the reference) the same next learning rate needs t + 1
            import warnings
            warnings.warn("LinearWarmupSchedule: loading a round-1-format scheduler state ('t'): it is read as written by the "
                          "scheduler-before-optimizer train loop of that round (t + 1); checkpoints written since carry 'last_epoch'")
            self.t, self.warm, self.total, self.base = sd["t"] + 1, sd["warm"], sd["total"], sd["base"]
        else:
            raise ValueError("scheduler state has neither 'last_epoch' nor 't': keys %s" % sorted(sd.keys()))
        self._apply()
