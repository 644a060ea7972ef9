"""Fused AdamW over libmnyolo's multi-tensor kernel — a drop-in for `torch.optim.AdamW` at train.py:134,283.

    optimizer = AdamW(model.parameters(), lr=7e-4, weight_decay=4e-4)      # same arguments as torch.optim.AdamW
    loss.backward(); optimizer.step()

One HIP launch per step updates every parameter (the reference issues ~200 small tensor updates).  State layout matches
torch's (`state[p] = {"step", "exp_avg", "exp_avg_sq"}`; the two moments are views into flat buffers), so
`state_dict()` / `load_state_dict()` interoperate with `torch.optim.AdamW` checkpoints.  Parameters whose `.grad` is
None are skipped exactly like upstream (the seg branch, Q10).  fp32 CUDA(HIP) parameters only; no CPU fallback.

`clip_grad_norm_(model_or_parameters, max_norm)` is `torch.nn.utils.clip_grad_norm_` (L2) in two launches on the same gradients
and without a host synchronisation (mny_grad_clip).

`SGD` is `torch.optim.SGD` (momentum, dampening, weight decay, Nesterov) the same way (mny_sgd_step); `ModelEMA` keeps an
exponential moving average of the weights in one flat shadow (mny_ema_update, one launch per step) and swaps it in place with the
live weights around evaluation (mny_swap_chunks), so the average needs no second module and no second plan.
"""
import collections
import contextlib
import ctypes
import math

import numpy as np
import torch

from . import _lib, dp

CHUNK = 65536
STREAM_CHUNK = 16384      # chunk length of the SGD / EMA / swap tables (a multiple of 4): see LAB_NOTES "SGD, EMA and swap launches"
_SEG_DT = np.dtype([("g", np.uint64), ("n", np.int64), ("block0", np.int32), ("pad", np.int32)])
_CHUNK_DT = np.dtype([("p", np.uint64), ("g", np.uint64), ("m", np.uint64), ("v", np.uint64), ("n", np.int32), ("vec4", np.int32)])


class AdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False):
        if amsgrad:
            raise _lib.MnyError("fused AdamW: amsgrad is not implemented (the reference does not use it)")
        if lr < 0 or eps < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1 or weight_decay < 0:
            raise ValueError("invalid AdamW hyper-parameters")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False))
        self._tables = {}           # group index -> (signature, [one chunk table per distinct step count: table, nchunks, t, params])

    def _ensure_state(self, group):
        new = [p for p in group["params"] if p.grad is not None and len(self.state[p]) == 0]
        if not new:
            return
        total = sum((p.numel() + 3) // 4 * 4 for p in new)
        dev = new[0].device
        flat_m = torch.zeros(total, device=dev, dtype=torch.float32)
        flat_v = torch.zeros(total, device=dev, dtype=torch.float32)
        off = 0
        for p in new:
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise _lib.MnyError("fused AdamW needs contiguous fp32 CUDA(HIP) parameters — there is no CPU fallback")
            n = p.numel()
            st = self.state[p]
            st["step"] = torch.tensor(0.0)
            st["exp_avg"] = flat_m[off:off + n].view_as(p)
            st["exp_avg_sq"] = flat_v[off:off + n].view_as(p)
            off += (n + 3) // 4 * 4

    def _table(self, gi, group):
        """Device chunk tables of group `gi`, rebuilt only when a parameter / gradient pointer changes (a step costs one pass
        over the parameters reading two pointers each — the moments only move through load_state_dict, which drops the cache).
        One table (= one launch) per distinct step count: torch keeps the step per parameter, and parameters that first receive
        a gradient later (a branch enabled or unfrozen mid-run, a torch checkpoint with mixed counts) carry their own."""
        live = [p for p in group["params"] if p.grad is not None]
        sig = tuple((p.data_ptr(), p.grad.data_ptr()) for p in live)
        cached = self._tables.get(gi)
        if cached is not None and cached[0] == sig:
            return cached[1], live
        self._sync_steps(gi)                                      # counters of the parameters the old tables covered
        by_step = {}
        for p, (pp, gp) in zip(live, sig):
            g, st = p.grad, self.state[p]
            if not (g.is_cuda and g.dtype == torch.float32 and g.is_contiguous()):
                raise _lib.MnyError("fused AdamW needs contiguous fp32 CUDA(HIP) gradients")
            mp, vp = st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
            n = p.numel()
            sub = by_step.setdefault(int(float(st["step"])), {"rows": [], "ids": set(), "params": []})
            sub["ids"].add(id(p))
            sub["params"].append(p)
            for o in range(0, n, CHUNK):
                c = min(CHUNK, n - o)
                ptrs = (pp + 4 * o, gp + 4 * o, mp + 4 * o, vp + 4 * o)
                sub["rows"].append(ptrs + (c, int(all(q % 16 == 0 for q in ptrs))))
        subs = []
        for t in sorted(by_step):
            sub = by_step[t]
            host = np.array(sub["rows"], dtype=_CHUNK_DT)
            subs.append({"table": torch.from_numpy(host.view(np.uint8).reshape(-1)).to(live[0].device), "nchunks": len(sub["rows"]), "t": t,
                         "ids": sub["ids"], "params": sub["params"]})
        self._tables[gi] = (sig, subs)
        return subs, live

    def _sync_steps(self, only=None):
        """write the step counters back into the per-parameter `step` tensors (torch's state layout)"""
        for gi in list(self._tables):
            if only is not None and gi != only:
                continue
            for sub in self._tables[gi][1]:
                for p in sub["params"]:
                    self.state[p]["step"].fill_(float(sub["t"]))

    def state_dict(self):
        self._sync_steps()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._tables.clear()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            self._ensure_state(group)
            if not any(p.grad is not None for p in group["params"]):
                continue
            subs, live = self._table(gi, group)
            b1, b2 = group["betas"]
            st = ctypes.c_void_p(torch.cuda.current_stream(live[0].device).cuda_stream)
            for sub in subs:                                      # normally one; one launch per distinct step count otherwise
                sub["t"] += 1
                _lib.call("mny_adamw_step", ctypes.c_void_p(sub["table"].data_ptr()), sub["nchunks"], float(group["lr"]), float(b1), float(b2),
                          float(group["eps"]), float(group["weight_decay"]), sub["t"], st)
        return loss


def _chunk_rows(ptrs, n, chunk):
    """mny_adamw_chunk rows of one tensor: `ptrs` = (p, g, m, v) addresses, 0 for a field the entry point does not use;
    vec4 = every address in use is 16-byte aligned (the chunk length is a multiple of 4, so a tensor's chunks share its alignment)."""
    rows = []
    for o in range(0, n, chunk):
        q = tuple(a + 4 * o if a else 0 for a in ptrs)
        rows.append(q + (min(chunk, n - o), int(all(a % 16 == 0 for a in q))))
    return rows


def _device_table(rows, dev):
    host = np.array(rows, dtype=_CHUNK_DT)
    return torch.from_numpy(host.view(np.uint8).reshape(-1)).to(dev)


def _fp32_device(t):
    return t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()


class SGD(torch.optim.Optimizer):
    """`torch.optim.SGD` (momentum, dampening, weight decay, Nesterov) in one launch per param group and state (mny_sgd_step).

        optimizer = SGD(model.parameters(), lr=1e-2, momentum=0.9, nesterov=True, weight_decay=5e-4)
        loss.backward(); optimizer.step()

    State layout is torch's (`state[p]["momentum_buffer"]`, views into one flat buffer), so `state_dict()` / `load_state_dict()`
    interoperate with `torch.optim.SGD` in both directions; a parameter without a buffer (none yet, or `None` in a torch checkpoint)
    takes torch's first-step form (`buf = d`) on a table of its own while the others run on.  Parameters whose `.grad` is None are
    skipped.  fp32 contiguous CUDA(HIP) parameters and gradients only, `maximize` is not implemented: both raise `MnyError`."""

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False):
        if maximize:
            raise _lib.MnyError("fused SGD: maximize is not implemented")
        if lr < 0.0:
            raise ValueError("Invalid learning rate: %s" % (lr,))
        if momentum < 0.0:
            raise ValueError("Invalid momentum value: %s" % (momentum,))
        if weight_decay < 0.0:
            raise ValueError("Invalid weight_decay value: %s" % (weight_decay,))
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        # (the last four keys are torch.optim.SGD's: a state_dict of this class then reads like one of torch's)
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                                      maximize=False, foreach=None, differentiable=False, fused=None))
        self._tables = {}           # group index -> (signature, [{"table", "nchunks", "first"}])
        self._first = set()         # ids of the parameters whose buffer exists but has not been written: their next step is a first step

    @staticmethod
    def _check(p):
        if not (_fp32_device(p) and _fp32_device(p.grad)):
            raise _lib.MnyError("fused SGD needs contiguous fp32 CUDA(HIP) parameters and gradients — there is no CPU fallback")

    def _new_buffers(self, live):
        """Momentum buffers for the parameters that have none: views into one flat buffer.  Those parameters' next step is torch's first
        step (buf = d), which writes the buffer without reading it."""
        new = [p for p in live if self.state[p].get("momentum_buffer") is None]
        if not new:
            return
        for p in new:
            self._check(p)
        flat = torch.zeros(sum((p.numel() + 3) // 4 * 4 for p in new), device=new[0].device, dtype=torch.float32)
        off = 0
        for p in new:
            n = p.numel()
            self.state[p]["momentum_buffer"] = flat[off:off + n].view_as(p)
            off += (n + 3) // 4 * 4
        self._first.update(id(p) for p in new)

    def _table(self, gi, live, mom):
        """Device chunk tables of group `gi`: one for the parameters on their first step, one for the running ones; rebuilt only when a
        parameter / gradient pointer moves or a parameter changes sides (the buffers only move through load_state_dict, which drops the cache)."""
        sig = (mom,) + tuple((p.data_ptr(), p.grad.data_ptr(), mom and id(p) in self._first) for p in live)
        cached = self._tables.get(gi)
        if cached is not None and cached[0] == sig:
            return cached[1]
        rows = {False: [], True: []}
        for p, (pp, gp, first) in zip(live, sig[1:]):
            self._check(p)
            mp = 0
            if mom:
                buf = self.state[p]["momentum_buffer"]
                if not (_fp32_device(buf) and buf.numel() == p.numel()):
                    raise _lib.MnyError("fused SGD: momentum_buffer must be a contiguous fp32 CUDA(HIP) tensor of the parameter's size")
                mp = buf.data_ptr()
            rows[first] += _chunk_rows((pp, gp, mp, 0), p.numel(), STREAM_CHUNK)
        subs = [{"table": _device_table(r, live[0].device), "nchunks": len(r), "first": int(first)} for first, r in rows.items() if r]
        self._tables[gi] = (sig, subs)
        return subs

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._tables.clear()
        self._first.clear()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            if group.get("maximize"):
                raise _lib.MnyError("fused SGD: maximize is not implemented")
            live = [p for p in group["params"] if p.grad is not None and p.numel()]
            if not live:
                continue
            mom = group["momentum"] != 0
            if mom:
                self._new_buffers(live)
            subs = self._table(gi, live, mom)
            st = ctypes.c_void_p(torch.cuda.current_stream(live[0].device).cuda_stream)
            for sub in subs:                                      # normally one launch; two while some parameters take their first step
                _lib.call("mny_sgd_step", ctypes.c_void_p(sub["table"].data_ptr()), sub["nchunks"], float(group["lr"]), float(group["momentum"]),
                          float(group["dampening"]), float(group["weight_decay"]), int(bool(group["nesterov"])), sub["first"], st)
            if mom and self._first:
                self._first.difference_update(id(p) for p in live)
        return loss


class ModelEMA:
    """Exponential moving average of a model's weights as ONE flat fp32 shadow, swapped in place with the live weights for evaluation.

        ema = ModelEMA(model, decay=0.9998, tau=2000)     # shadow of every floating-point state_dict entry (parameters AND BN running stats)
        loss.backward(); opt.step(); ema.update()          # one launch (mny_ema_update)
        with ema.applied():                                # one swap launch in, one out (mny_swap_chunks)
            detections = model.eval()(images)              # same tensors, same pointers: no plan is rebuilt
        ema.copy_to_model()                                # end of training: overwrite the live weights

    `update()` counts `updates += 1` and averages with d = decay * (1 - exp(-updates / tau)) (the warm-up of YOLOv5's ModelEMA); tau 0 or
    None: d = decay.  Integer entries (`num_batches_tracked`) are never averaged or swapped.  No second module, no second plan: the cost is
    one parameter-sized buffer.  Under data parallel nothing more is needed — after `optimizer.step()` the parameters are identical on every
    rank, hence the shadows too.  fp32 contiguous CUDA(HIP) tensors only: `update()` and `applied()` raise `MnyError` otherwise."""

    def __init__(self, model, decay=0.9998, tau=2000):
        if not 0.0 <= decay <= 1.0:
            raise ValueError("Invalid EMA decay: %s" % (decay,))
        if tau is not None and tau < 0:
            raise ValueError("Invalid EMA tau: %s" % (tau,))
        self.model, self.decay, self.tau, self.updates = model, float(decay), tau, 0
        self._applied = False
        self._tab = None            # (signature, device table, nchunks)
        # holders of the floating-point state_dict entries, in state_dict order: the module tree is walked once, the tensors are looked
        # up at every call (Module.to() replaces buffer objects)
        self._slots = []            # (name, the module's _parameters / _buffers dict, key, offset, numel)
        off = 0
        for mname, mod in model.named_modules():
            for kind in ("_parameters", "_buffers"):
                for key, t in getattr(mod, kind).items():
                    if t is None or (kind == "_buffers" and key in mod._non_persistent_buffers_set) or not t.is_floating_point():
                        continue
                    self._slots.append((mname + "." + key if mname else key, getattr(mod, kind), key, off, t.numel()))
                    off += (t.numel() + 3) // 4 * 4
        sd = model.state_dict()
        if [s[0] for s in self._slots] != [k for k, v in sd.items() if v.is_floating_point()]:
            raise _lib.MnyError("ModelEMA: the module's parameters and persistent buffers do not line up with its state_dict() entries")
        live = self._live()
        if not live:
            raise _lib.MnyError("ModelEMA: the model has no floating-point state")
        if any(t.dtype != torch.float32 or t.device != live[0].device for t in live):
            raise _lib.MnyError("ModelEMA needs fp32 state on one device")
        self._flat = torch.zeros(off, device=live[0].device, dtype=torch.float32)
        torch._foreach_copy_(self._views(), [t.detach() for t in live])

    def _live(self):
        return [holder[key] for _nm, holder, key, _off, _n in self._slots]

    def _views(self, like=None):
        like = like or self._live()
        return [self._flat[off:off + n].view_as(t) for (_nm, _holder, _key, off, n), t in zip(self._slots, like)]

    def decay_at(self, updates):
        """The averaging coefficient of update number `updates` (1-based)."""
        return self.decay * (1.0 - math.exp(-updates / self.tau)) if self.tau else self.decay

    def _table(self):
        """(device chunk table, nchunks, device), cached on the pointer signature like AdamW._table: `model.to(...)`, or anything else that
        moves a tensor, rebuilds it (the shadow follows the model to its device)."""
        live = self._live()
        sig = tuple(t.data_ptr() for t in live)
        if self._tab is not None and self._tab[0] == sig:
            return self._tab[1:]
        dev = live[0].device
        if not all(_fp32_device(t) and t.device == dev for t in live):
            raise _lib.MnyError("ModelEMA needs contiguous fp32 CUDA(HIP) state on one device — there is no CPU fallback")
        if len(set(sig)) != len(sig):
            raise _lib.MnyError("ModelEMA: two state_dict entries share storage (tied weights are not supported)")
        if self._flat.device != dev:
            if self._applied:
                raise _lib.MnyError("ModelEMA: the model moved to another device inside applied()")
            self._flat = self._flat.to(dev)
        base, rows = self._flat.data_ptr(), []
        for (_nm, _holder, _key, off, n), pp in zip(self._slots, sig):
            rows += _chunk_rows((pp, 0, base + 4 * off, 0), n, STREAM_CHUNK)
        self._tab = (sig, _device_table(rows, dev), len(rows), dev)
        return self._tab[1:]

    def _launch(self, name, *args):
        table, nchunks, dev = self._table()
        _lib.call(name, ctypes.c_void_p(table.data_ptr()), nchunks, *args, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))

    def _not_applied(self, what):
        if self._applied:
            raise _lib.MnyError("ModelEMA.%s inside applied(): the live weights are the shadow's right now" % what)

    @torch.no_grad()
    def update(self):
        self._not_applied("update()")
        self._table()                                             # (every refusal before the counter moves)
        self.updates += 1
        self._launch("mny_ema_update", float(self.decay_at(self.updates)))

    @contextlib.contextmanager
    def applied(self):
        """Evaluate (or checkpoint `model.state_dict()`) under the averaged weights: the shadow and the live tensors exchange contents in
        place, and exchange them back on exit."""
        if self._applied:
            raise _lib.MnyError("ModelEMA.applied() is already active (it does not nest)")
        for plan in getattr(self.model, "_plans", {}).values():
            if getattr(plan, "inflight_gen", None) is not None:
                raise _lib.MnyError("ModelEMA.applied(): a differentiable forward of this model still awaits its backward — its saved "
                                    "activations belong to the raw weights; call backward() (or drop the losses) first")
        self._launch("mny_swap_chunks")
        self._applied = True
        try:
            yield self.model
        finally:
            self._launch("mny_swap_chunks")
            self._applied = False

    @torch.no_grad()
    def copy_to_model(self):
        """Overwrite the live weights (and BN running statistics) with the average."""
        self._not_applied("copy_to_model()")
        live = self._live()
        torch._foreach_copy_([t.detach() for t in live], [v.to(live[0].device) for v in self._views(live)])

    def shadow_state_dict(self):
        """A state dict `model.load_state_dict` accepts: float entries from the shadow, integer entries (`num_batches_tracked`) copied from
        the model at call time."""
        self._not_applied("shadow_state_dict()")
        shadow = dict(zip((s[0] for s in self._slots), self._views()))
        return collections.OrderedDict((k, (shadow[k] if k in shadow else v.detach()).clone()) for k, v in self.model.state_dict().items())

    def state_dict(self):
        self._not_applied("state_dict()")
        return {"updates": self.updates, "decay": self.decay, "tau": self.tau,
                "shadow": collections.OrderedDict((s[0], v.clone()) for s, v in zip(self._slots, self._views()))}

    @torch.no_grad()
    def load_state_dict(self, state):
        self._not_applied("load_state_dict()")
        views, shadow = self._views(), state["shadow"]
        if list(shadow) != [s[0] for s in self._slots] or any(tuple(shadow[s[0]].shape) != tuple(v.shape) for s, v in zip(self._slots, views)):
            raise _lib.MnyError("ModelEMA.load_state_dict: the shadow's entries do not match this model's floating-point state")
        torch._foreach_copy_(views, [shadow[s[0]].to(device=self._flat.device, dtype=torch.float32) for s in self._slots])
        self.updates, self.decay, self.tau = int(state["updates"]), float(state["decay"]), state["tau"]


def clip_segment_table(segments):
    """[(address, floats)] -> (host table of mny_clip_seg rows, total blocks): each segment's blocks follow its predecessor's."""
    rows, nblocks = [], 0
    for ptr, n in segments:
        rows.append((ptr, n, nblocks, 0))
        nblocks += _lib.query("mny_grad_clip_parts", n)
    return np.array(rows, dtype=_SEG_DT), nblocks


_clip_cache = {}          # device -> (signature, segment table, workspace, out): rebuilt only when a gradient pointer changes


def clip_grad_norm_(parameters, max_norm):
    """`torch.nn.utils.clip_grad_norm_(parameters, max_norm)` with the L2 norm: scales every `.grad` in place by
    min(1, max_norm / (total_norm + 1e-6)) and returns total_norm as a 0-dim device tensor — two launches (mny_grad_clip), no host
    synchronisation; a non-finite norm propagates into the gradients as it does upstream.  `parameters`: an iterable of parameters, one
    parameter, or a module; pending all-reduces of models with data-parallel gradients attached (dp.attach_data_parallel) are waited for
    first, in every one of these forms, so the AVERAGED gradients are clipped.  The gradients may be the model's arena views or any other contiguous fp32 CUDA(HIP) tensors; each
    one is a segment of its own, so the padding between arena slots never enters the norm."""
    dp.wait_pending()               # averaged gradients, whichever way the parameters were handed over (no reducer attached: nothing to wait for)
    if isinstance(parameters, torch.nn.Module):
        parameters = parameters.parameters()
    elif isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return torch.tensor(0.0)
    for g in grads:
        if not (g.is_cuda and g.dtype == torch.float32 and g.is_contiguous()):
            raise _lib.MnyError("clip_grad_norm_ needs contiguous fp32 CUDA(HIP) gradients (got %s on %s) — there is no CPU fallback" % (g.dtype, g.device))
    dev = grads[0].device
    if any(g.device != dev for g in grads):
        raise _lib.MnyError("clip_grad_norm_: gradients on several devices")
    sig = tuple((g.data_ptr(), g.numel()) for g in grads if g.numel())
    if not sig:
        return torch.zeros((), device=dev)
    cached = _clip_cache.get(dev)
    if cached is None or cached[0] != sig:
        host, nblocks = clip_segment_table(sig)
        table = torch.from_numpy(host.view(np.uint8).reshape(-1)).to(dev)
        cached = _clip_cache[dev] = (sig, table, torch.empty(nblocks, device=dev, dtype=torch.float64), torch.empty(2, device=dev, dtype=torch.float32), nblocks)
    _, table, ws, out, nblocks = cached
    with torch.cuda.device(dev):
        _lib.call("mny_grad_clip", ctypes.c_void_p(table.data_ptr()), len(sig), nblocks, float(max_norm), ctypes.c_void_p(ws.data_ptr()),
                  ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        return out[0].clone()               # (the two result floats are reused by the next call)
