"""Static execution plans for the MobileNet-YOLO graph: one flat list of C-ABI calls for the forward
pass, one for the backward pass, built once per (batch, height, width, mode) and replayed every step.

All device buffers (raw conv outputs, BN coefficients, gradients, workspaces) are allocated when the
plan is built and stay resident — at bs=256/352x352 that is ~60 GB of the 288 GB HBM — so a step does
no allocation, no host<->device synchronisation and no Python work besides walking the call list
(which is also what makes the whole step hipGraph-capturable).

Backward dataflow (per conv+BN+act unit, given G = dL/d(activated output)):
    bn_bwd_reduce(G, Y) -> bn_bwd_finalize -> dgamma, dbeta, coef ; bn_bwd_apply -> dY
    wgrad(view(input), dY) -> dW        dgrad(dY, W) (+ addend) -> G of the input
Residual adds alias G to both operands; a second contribution to a value is fused into the producing
kernel's `addend` epilogue, so no separate accumulation pass exists.

The plan compiler (NetPlan): one graph analysis (_analyse_graph), the unit matching (_match_exdw, _match_gates), then per node one
emitter.  Forward: _FWD (_fwd_unit with _fwd_stem / _fwd_dw / _fwd_exdw_dw / _fwd_exdw_pw / _fwd_pw, _fwd_head, _fwd_add, _fwd_mul,
_fwd_partadd) and _emit_gate_forward.  Backward: _bwd_emitter picks _bwd_gate, _bwd_exdw, _bwd_add, _bwd_mul, _bwd_partadd,
_bwd_thin_expand, _bwd_lr_expand, _bwd_dw_s1, _bwd_dw_s2, _bwd_dw_s2k5, _bwd_project or _bwd_generic (_bwd_dw_grads / _bwd_pw_grads);
the steps they share are _bn_sums, _wgrad_dest, _sole_producer, _red_target, _accumulate_into / _contribute_alias / _contribute_kernel.
"""
import ctypes
import itertools
import os
import re
import warnings

import numpy as np
import torch

from . import _lib, frontier, switches
from ._lib import ACT_NONE, MnyError, YoloHead

_FWD_TICK = itertools.count()            # process-wide order of training forwards (NetPlan.last_fwd_tick)

BN_EPS = 1e-5
BN_MOMENTUM = 0.1
_vp = ctypes.c_void_p


def _ptr(t):
    return _vp(t.data_ptr()) if t is not None else None


class CallList:
    """A replayable sequence of C-ABI calls."""

    def __init__(self):
        self.calls = []
        self.keep = []           # tensors referenced by raw pointers
        self.marks = {}          # name -> call index (for DP bucket events)

    def add(self, name, *args, meta=None, label=None):
        """`label`: the entry point this call stands for in timing tables / launch fingerprints (the _w6 twins of the GEMM entry points)."""
        fn = getattr(_lib.load(), name)
        conv = []
        for a in args:
            if isinstance(a, torch.Tensor):
                assert a.is_contiguous() and a.is_cuda, name
                self.keep.append(a)
                conv.append(_vp(a.data_ptr()))
            else:
                conv.append(a)
        self.calls.append((fn, tuple(conv), label or name, meta))   # meta: algorithmic {flops, bytes} of the call

    def add_py(self, fn, name="py"):
        """A host-side step of the list (stream fork / join): any callable returning None."""
        self.calls.append((fn, (), name, None))

    def run(self, begin=0, end=None):
        lib = _lib.load()
        for fn, args, name, _ in self.calls[begin:end]:
            rc = fn(*args)
            if rc:
                raise MnyError("%s failed (%d): %s" % (name, rc, lib.mny_last_error().decode()))

    def run_recording(self, routes, begin=0, end=None):
        """run(), and for every pointwise-conv call note the kernel family its dispatcher took (mny_pw_last_route) in routes[call index]."""
        lib = _lib.load()
        end = len(self.calls) if end is None else end
        for idx in range(begin, end):
            fn, args, name, _ = self.calls[idx]
            rc = fn(*args)
            if rc:
                raise MnyError("%s failed (%d): %s" % (name, rc, lib.mny_last_error().decode()))
            if name.startswith(("mny_pw_fwd", "mny_pw_dgrad_bnred", "mny_pw_wgrad")):
                routes[idx] = lib.mny_pw_last_route()

    def run_timed(self, events, only=None, begin=0, end=None):
        """Like run(), bracketing each call (or only the entry points named in `only`) with HIP events
        recorded on torch's current stream — the stream the kernels are launched on.
        Appends (call index, name, start, end) to `events`."""
        lib = _lib.load()
        end = len(self.calls) if end is None else end
        stream = _vp(torch.cuda.current_stream().cuda_stream)
        for idx in range(begin, end):
            fn, args, name, _ = self.calls[idx]
            timed = only is None or name in only
            if timed:
                a, b = HipEvent.take(), HipEvent.take()
                a.record(stream)
            rc = fn(*args)
            if rc:
                raise MnyError("%s failed (%d): %s" % (name, rc, lib.mny_last_error().decode()))
            if timed:
                b.record(stream)
                events.append((idx, name, a, b))


class _TorchEvent:
    """Fallback bracket event (see HipEvent._new)."""
    __slots__ = ("e",)

    def __init__(self):
        self.e = torch.cuda.Event(enable_timing=True)

    def record(self, stream):
        self.e.record()

    def elapsed_time(self, other):
        return self.e.elapsed_time(other.e)


class HipEvent:
    """Timing events straight on the HIP runtime (hipEventCreate / hipEventRecord / hipEventElapsedTime through ctypes), drawn from
    a pool that is filled BEFORE the timed region: a `torch.cuda.Event` is created lazily inside its first `record()`, which put
    ~10 us of host work per bracket into the measured step (invisible at bs=256, 15 % of the step at bs=64)."""
    _hip = None
    _checked = False
    _pool = []
    _next = 0
    __slots__ = ("h",)

    @classmethod
    def _rt(cls):
        if cls._hip is None:
            path = "libamdhip64.so"
            try:                                   # the copy of the runtime TORCH runs on: a handle from another mapped copy crashes instead of failing
                tlib = os.path.join(os.path.dirname(os.path.abspath(torch.__file__)), "lib")
                cands = []
                with open("/proc/self/maps") as f:
                    for line in f:
                        if "libamdhip64.so" in line:
                            cands.append(line.split()[-1])
                mine = [c for c in cands if os.path.dirname(os.path.abspath(c)) == tlib]
                uniq = sorted(set(cands))
                if mine:
                    path = mine[0]                 # torch's bundled runtime
                elif len(uniq) == 1:
                    path = uniq[0]                 # one runtime in the process (system ROCm): unambiguous
                elif uniq:
                    raise OSError("several HIP runtimes mapped (%s), none of them torch's" % ", ".join(uniq))
            except OSError as e:
                warnings.warn("raw HIP events unavailable (%s); timing brackets use torch.cuda.Event" % (e,))
                cls._hip = False
                raise MnyError("no unambiguous HIP runtime")
            cls._hip = ctypes.CDLL(path)
            cls._hip.hipEventCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
            cls._hip.hipEventRecord.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
            cls._hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
        return cls._hip

    def __init__(self):
        h = ctypes.c_void_p()
        if self._rt().hipEventCreate(ctypes.byref(h)) != 0:
            raise MnyError("hipEventCreate failed")
        self.h = h

    @classmethod
    def _new(cls):
        """A raw HIP event; if the runtime cannot be reached through ctypes (or is not the one torch runs on), a torch event."""
        if cls._hip is not False:
            try:
                ev = cls()
                if not cls._checked:               # one record / elapsed round trip on torch's stream before trusting the handle
                    ev2 = cls()
                    st = _vp(torch.cuda.current_stream().cuda_stream)
                    ev.record(st); ev2.record(st)
                    torch.cuda.current_stream().synchronize()
                    ev.elapsed_time(ev2)
                    cls._checked = True
                return ev
            except (OSError, AttributeError, MnyError, RuntimeError) as e:
                warnings.warn("raw HIP events unavailable (%s); timing brackets fall back to torch.cuda.Event" % (e,))
                cls._hip = False
        return _TorchEvent()

    @classmethod
    def reserve(cls, n):
        """Rewind the pool and make sure it holds n events (call outside the timed region)."""
        cls._next = 0
        while len(cls._pool) < n:
            cls._pool.append(cls._new())

    @classmethod
    def take(cls):
        if cls._next == len(cls._pool):
            cls._pool.append(cls._new())
        cls._next += 1
        return cls._pool[cls._next - 1]

    def record(self, stream):
        if self._hip.hipEventRecord(self.h, stream) != 0:
            raise MnyError("hipEventRecord failed")

    def elapsed_time(self, other):
        ms = ctypes.c_float()
        if self._hip.hipEventElapsedTime(ctypes.byref(ms), self.h, other.h) != 0:
            raise MnyError("hipEventElapsedTime failed (events not complete?)")
        return float(ms.value)


class _Unit:
    """Resident state of one conv+BN+act unit."""
    __slots__ = ("Y", "coef4", "scale", "shift", "mean", "invstd", "act", "C", "M", "shape")


class _Grad:
    """Gradient buffer of one value while the backward list is built; `shared`: the buffer is also another value's gradient (an alias)."""
    __slots__ = ("buf", "shared")

    def __init__(self):
        self.buf, self.shared = None, False


_NO_VIEW = (None, None, None, ACT_NONE)
_HARD = (_lib.ACT_HSWISH, _lib.ACT_HSIGMOID)


class NetPlan:
    def __init__(self, net, N, H, W, training, act_dtype=torch.float32, bn_batch=None, frozen_bwd=False, frozen_params=(), bn_eval=()):
        """training: build the loss calls (else decode + NMS).  bn_batch (default = training): BatchNorm on batch statistics
        with the running-statistics update, and the backward list; False with training=True is the "validation loss" plan
        (running statistics, buffers untouched) — forward only, or with frozen_bwd the backward list of frozen BatchNorm
        (the statistics are constants of the step: mbv2_yolo.py:157 under model.eval() with gradients).
        frozen_params: names of the parameters with requires_grad == False — the backward list stops at the frontier they leave
        (frontier.py) and the gradient arena lists only the others.  bn_eval: names of the BatchNorm modules in eval mode while the plan
        runs on batch statistics: those units normalise with their running statistics and update nothing (below the frontier only)."""
        self.net, self.N, self.H, self.W, self.training = net, N, H, W, training
        bn_batch = training if bn_batch is None else bool(bn_batch)      # (bn_batch without training: decode + NMS on batch statistics, model.train()(images))
        self.bn_batch = bn_batch
        self.frozen = bool(training and not bn_batch and frozen_bwd)
        self.frontier = frontier.Frontier(net.graph, frozen_params)
        self.bn_eval = frozenset(bn_eval) if bn_batch else frozenset()
        if training and bn_batch:
            frontier.check_bn_modes(net.graph, self.frontier, self.bn_eval)
        self.fwd_gen = 0
        self.inflight_gen = None                # model._InFlight: forward generation whose backward is still owed
        self.last_fwd_tick = -1                 # process-wide order of training forwards (model._grad_plan picks the oldest when every slot is busy)
        self.resident_bytes = 0
        dev = net.device
        self.dev = dev
        # storage type of activations / activation gradients.  bf16 selects the `*_bf16` twins of the entry points
        # (same arithmetic in fp32 registers, half the HBM bytes); weights, BN statistics, parameter gradients and the
        # detection heads seen by loss / decode stay fp32.
        assert act_dtype in (torch.float32, torch.bfloat16), act_dtype
        # every switch the plan compiler knows (switches.py), read here, once per plan
        sw_hipgraph, sw_side, sw_exdw_k, sw_no_gate = (switches.get(n) for n in ("MNY_HIPGRAPH", "MNY_SIDE_STREAM", "MNY_EXDW_K", "MNY_NO_GATE"))
        self.sw_no_lr, self.sw_no_lr_s2, self.sw_no_dwfuse5s2 = (switches.get(n) for n in ("MNY_NO_LR", "MNY_NO_LR_S2", "MNY_NO_DWFUSE5S2"))
        self.adt = act_dtype
        self.bf16 = act_dtype == torch.bfloat16
        self.eb = 2 if self.bf16 else 4
        assert H % 32 == 0 and W % 32 == 0, "input height/width must be multiples of 32 (got %dx%d)" % (H, W)
        g = net.graph
        self.stream = _vp(0)
        self.x_ptr = _vp(0)
        self.timing = None
        self.routes = {"fwd": {}, "bwd": {}}     # call index -> kernel family the dispatcher actually took (recorded at the first replay)
        self._recorded = set()                   # (which, begin, end) segments whose first replay has been recorded
        self.reducer = None
        # optional hipGraph replay (MNY_HIPGRAPH=1): after two eager steps (which also run every one-time HIP attribute /
        # occupancy query) the call lists are captured once per segment and replayed.  Measured on MI355X: no gain
        # (68.1 vs 67.7 ms/step) — the eager list already keeps the GPU queue full — so it is off by default.
        self.use_graphs = training and sw_hipgraph
        # weight-gradient kernels on a side stream: they feed nothing downstream in the backward pass, so they can overlap the
        # kernels of the following layers.  Fork = the side stream waits for what the main stream has enqueued (dY ready); join
        # before every batched combine and at the end of every replayed segment.  Measured (same-box A/B): no gain at
        # bs=256/352x352, where every kernel fills the chip (49.4 vs 49.5-49.8 ms), +3 % on MobileNetV3 512x512 bs=64 bf16, whose
        # 10-100 us kernels leave CUs idle (17.7 -> 17.2 ms).  Round 4 (same-box, un-bracketed steps): bs 256 / 352x352 38.19 -> 37.98 and
        # 38.07 -> 37.91 ms, so it is on up to 48 M input pixels; fewer resident depthwise-backward workgroups to make room for the side
        # kernels lose more than the overlap gains (512 instead of 768: +0.3 ms).  A step whose launches are bracketed with HIP events runs
        # single-stream (the brackets must mean something): bench.py brackets every 4th timed step (--bracket-every), so three quarters of
        # the steps behind its `value` run with the side stream, one quarter without.  MNY_SIDE_STREAM=0/1 forces.
        auto_side = N * H * W <= 48 * 1000 * 1000
        self.side_on = training and not self.use_graphs and (sw_side == 1 or (sw_side is None and auto_side))
        self.stream_side = _vp(0)
        self._side_stream = torch.cuda.Stream(dev) if self.side_on else None
        self._ev_fork = torch.cuda.Event() if self.side_on else None
        self._ev_join = torch.cuda.Event() if self.side_on else None
        # a second side stream for the SHORT dependent kernels of the low-rank BN backward (mny_lr_prep): they must not queue behind the weight
        # gradients of the first one, and the main stream waits for exactly them (its own event pair)
        self.stream_side2 = _vp(0)
        self._side2_stream = torch.cuda.Stream(dev) if self.side_on else None
        self._ev_fork2 = torch.cuda.Event() if self.side_on else None
        self._ev_join2 = torch.cuda.Event() if self.side_on else None
        self._side_used = False
        self.graphs = {}
        self.eager_steps = 0
        self.x_static = None
        self.fwd = CallList()
        self.bwd = None
        self._cvt_jobs = []
        self._cut_jobs = []           # (fp32 matrix, plane buffer): weights of the six-product GEMMs, cut once per pass (mny_cut3_batch)
        self.wT, self.wT6 = {}, {}    # conv name -> W^T of a generic pointwise unit / its pre-cut planes (backward data gradients)
        self._loss_side = False       # the first head's loss runs on the side stream (_build_detection)
        self._head0_call = None       # the forward call behind which the first head exists
        self.head32 = {}         # bf16 storage: value id -> fp32 copy of a detection head
        self.units = {}          # value id -> _Unit
        self.reals = {}          # value id -> tensor
        self._f32 = dict(device=dev, dtype=torch.float32)
        self._act = dict(device=dev, dtype=self.adt)
        self._P = net.param_tensors
        self.max_parts = _lib.query("mny_max_parts")
        self.maxC = max(v.C for v in g.values)
        self.stats_ws = torch.empty(self.max_parts * 2 * self.maxC, **self._f32)
        self.param_ptrs = [(t, t.data_ptr()) for t in net.all_state_tensors()]
        self._analyse_graph(g)
        self._match_exdw(g, sw_exdw_k)
        self._match_gates(g, sw_no_gate)
        for pid, d in self.exdw_pw.items():          # fused multi-BatchNorm units of the forward pass: their members share one mode
            frontier.check_fused_pair([g.values[pid].node.bn, d.bn], self.bn_eval, "expand + depthwise")
        for gate in self.gates.values():
            frontier.check_fused_pair([gate["se0"].bn, gate["se3"].bn], self.bn_eval, "gate")
        # Nodes no loss (or detection output) depends on — MobileNetV2-YOLO's always-on seg branch under a config without a `seg` section
        # (mbv2_yolo.py:155-156: computed, BatchNorm running statistics updated, result dropped) — feed nothing on the main stream: in a
        # training plan they run on the SIDE stream next to the rest of the forward pass (their own statistics workspace), joined behind the heads.
        self.dead_side = bool(self.side_on and bn_batch
                              and any(nd.out.id not in self.live and nd.op in ("dw", "pw", "add") for nd in g.nodes))
        self.stats_ws_side = torch.empty(self.max_parts * 2 * self.maxC, **self._f32) if self.dead_side else self.stats_ws
        dead_forked = self._build_forward(g)
        self._flush_cvt_jobs()
        self._flush_cut_jobs(self.fwd, at_head=True)
        self._flush_gate_jobs()
        self.heads = [self.head32.get(o.id, self.reals[o.id]) for o in g.outputs]
        self.seg_head = self.head32.get(g.seg_out.id, self.reals[g.seg_out.id]) if g.seg_out is not None else None
        self._build_detection()
        if dead_forked or self._loss_side:
            self.fwd.add_py(self._join_side, "join")                    # the dead branch's tensors (and the workspace it used) are free again before anything reuses them
        if training and (bn_batch or self.frozen) and self.frontier.order:      # (nothing trainable a loss depends on: forward only)
            self._build_backward(g)

    def _shape(self, v):
        return (self.N, self.H // v.down, self.W // v.down, v.C)

    def _rows(self, v):
        """Pixels of a value over the batch: the M of its GEMMs."""
        shp = self._shape(v)
        return shp[0] * shp[1] * shp[2]

    def _view(self, v):
        if v.kind == "unit":
            u = self.units[v.id]
            assert u.Y is not None, "%s is the un-materialised expand output of an exdw unit" % v.name
            return (u.Y, u.scale, u.shift, v.act)
        return (self.reals[v.id], None, None, ACT_NONE)

    # ---- graph analysis and unit matching ----------------------------------------------------------
    def _analyse_graph(self, g):
        """Everything the matching rules and both emission passes ask of the graph, computed once."""
        self.loss_outputs = list(g.outputs) + ([g.seg_out] if g.seg_out is not None else [])     # values a loss reads
        self.out_ids = {v.id for v in self.loss_outputs}
        self.consumers = {}                      # value id -> consumer nodes, in graph order
        for nd in g.nodes:
            for v in nd.ins:
                self.consumers.setdefault(v.id, []).append(nd)
        self.n_consumers = {v.id: len(self.consumers.get(v.id, ())) for v in g.values}           # ... counting the losses
        for v in self.loss_outputs:
            self.n_consumers[v.id] += 1
        self.live = set()                        # values a loss (or detection output) depends on
        stack = list(self.loss_outputs)
        while stack:
            v = stack.pop()
            if v.node is None or v.id in self.live:
                continue
            self.live.add(v.id)
            stack.extend(v.node.ins)
        self.bwd_order = [nd for nd in reversed(g.nodes) if nd.out.id in self.live]
        self.last_consumer = {}                  # value id -> the consumer node whose backward runs LAST (order = reverse topological)
        for nd in self.bwd_order:
            for v in nd.ins:
                self.last_consumer[v.id] = nd

    def _match_exdw(self, g, sw_exdw_k):
        """expand + depthwise units (csrc/exdw.hip): a thin expand conv (16 / 24 / 32 -> 6x channels, ReLU6) whose ONLY consumer is a 3x3
        stride-2 depthwise conv (ReLU6) runs as one unit that never writes the 6x-wide tensor or its gradient: every pass recomputes it
        from the thin input.  exdw_pw[expand node out id] = depthwise node, exdw_dw[depthwise node out id] = expand node."""
        self.exdw_pw, self.exdw_dw = {}, {}
        if self.bf16 or self.frozen:                    # (the frozen-BatchNorm backward runs on the generic, materialised kernels)
            return
        ks = set(int(v) for v in sw_exdw_k.split(",") if v)
        for nd in g.nodes:
            if nd.op != "pw" or nd.out.id in self.out_ids or len(self.consumers.get(nd.out.id, ())) != 1:
                continue
            d = self.consumers[nd.out.id][0]
            i = nd.ins[0]
            ish = self._shape(i)
            if (d.op == "dw" and d.k == 3 and d.stride == 2 and nd.out.act == _lib.ACT_RELU6 and d.out.act == _lib.ACT_RELU6 and not nd.bias
                    and i.act in (ACT_NONE, _lib.ACT_RELU6, _lib.ACT_LEAKY, _lib.ACT_RELU) and i.C in ks
                    and _lib.query("mny_exdw_supported", self.N, ish[1], ish[2], i.C, nd.out.C, 2) == 1):
                self.exdw_pw[nd.out.id] = d
                self.exdw_dw[d.out.id] = nd

    def _match_gates(self, g, sw_no_gate):
        """per-pixel gates as one unit (csrc/gate.hip, bf16 storage): t -> pw(C -> C/4, ReLU) -> pw(C/4 -> C, h-sigmoid) -> t * gate [-> + shortcut]
        (mobilenetv3.py:26-41,69-72).  gates[emit node out id] = dict(t, se0, se3, mul, add): the two hidden units are skipped where they stand
        and the whole unit is emitted at the multiply (or, when the residual add is its only consumer, at the add, which it absorbs)."""
        self.gates, self.gate_units, self.gate_absorbed = {}, {}, set()
        if not self.bf16 or self.frozen or sw_no_gate:
            return
        cons, out_ids = self.consumers, self.out_ids
        for nd in g.nodes:
            if nd.op != "mul":
                continue
            tv_, sv = nd.ins
            se3 = sv.node
            se0 = se3.ins[0].node if (se3 is not None and se3.op == "pw") else None
            if (se0 is None or se0.op != "pw" or se0.ins[0] is not tv_ or tv_.kind != "unit" or tv_.act != ACT_NONE or sv.act != _lib.ACT_HSIGMOID
                    or se0.out.act != _lib.ACT_RELU or se0.bias or se3.bias or len(cons.get(se0.out.id, ())) != 1 or len(cons.get(sv.id, ())) != 1
                    or len(cons.get(tv_.id, ())) != 2 or tv_.id in out_ids or se0.out.id in out_ids or sv.id in out_ids or nd.out.id in out_ids):
                continue                                    # (t feeds the gate and the multiply, nothing else: the unit's backward yields its whole gradient)
            tsh = self._shape(tv_)
            if _lib.query("mny_gate_supported", tsh[0] * tsh[1] * tsh[2], tv_.C, se0.out.C) != 1:
                continue
            gate = dict(t=tv_, se0=se0, se3=se3, mul=nd, add=None,
                        wq=torch.empty(int(_lib.query("mny_gate_wq_bytes", tv_.C, se0.out.C)), device=self.dev, dtype=torch.uint8))
            emit_at = nd
            mc = cons.get(nd.out.id, [])
            if len(mc) == 1 and mc[0].op == "add" and mc[0].k == 1 and mc[0].ins[0] is nd.out:
                gate["add"] = mc[0]                         # out = t * gate + view(other operand): the add node is absorbed
                emit_at = mc[0]
                self.gate_absorbed.add(nd.out.id)
            self.gates[emit_at.out.id] = gate
            self.gate_units[se0.out.id] = gate
            self.gate_units[se3.out.id] = gate

    # ---- forward list ------------------------------------------------------------------------------
    def _build_forward(self, g):
        """One emitter per node (_FWD); -> whether a dead branch was forked onto the side stream."""
        dead_forked = False
        for nd in g.nodes:
            o = nd.out
            dead = (self.dead_side and o.id not in self.live and nd.op in ("dw", "pw", "add")
                    and o.id not in self.exdw_pw and o.id not in self.exdw_dw)
            st = self.stream_side if dead else self.stream            # the stream and statistics workspace of this node's calls
            sws = self.stats_ws_side if dead else self.stats_ws
            if dead and not dead_forked:
                self.fwd.add_py(self._fork_side, "fork")                # the side stream waits for what the main stream has enqueued (the branch's input)
                dead_forked = True
            if nd.op == "pw" and o.id in self.gate_units:
                self._new_unit(o, materialise=False)          # a hidden unit of a gate: its BN coefficients live here, the calls come with the gate
            elif o.id in self.gate_absorbed:
                pass                                          # the multiply of a gate whose residual add absorbs it
            elif o.id in self.gates:
                self._emit_gate_forward(self.gates[o.id], nd)
            elif nd.op in self._FWD:
                self._FWD[nd.op](self, nd, st, sws)
            else:
                raise AssertionError(nd.op)
        return dead_forked

    def _new_unit(self, o, materialise=True):
        shp = self._shape(o)
        u = _Unit()
        u.Y = torch.empty(shp, **self._act) if materialise else None
        u.coef4 = torch.empty(4, o.C, **self._f32)
        u.scale, u.shift, u.mean, u.invstd = u.coef4[0], u.coef4[1], u.coef4[2], u.coef4[3]
        u.act, u.C, u.M, u.shape = o.act, o.C, shp[0] * shp[1] * shp[2], shp
        self.units[o.id] = u
        return u

    def _new_real(self, o):
        t = torch.empty(self._shape(o), **self._act)
        self.reals[o.id] = t
        return t

    def _batch_stats(self, bn):
        """Does the BatchNorm module `bn` normalise with (and update its running statistics from) the batch's statistics in this plan?"""
        return self.bn_batch and bn not in self.bn_eval

    def _emit_bn_tail(self, bn, u, parts, M, sws, st):
        """Behind a unit's forward conv: batch statistics -> coefficients and running statistics, or the coefficients of the running ones."""
        P = self._P
        gam, bet, rm, rv = P[bn + ".weight"], P[bn + ".bias"], P[bn + ".running_mean"], P[bn + ".running_var"]
        if self._batch_stats(bn):
            self.fwd.add("mny_bn_finalize", sws, parts, M, gam, bet, BN_EPS, BN_MOMENTUM, rm, rv, u.scale, u.shift, u.mean, u.invstd, u.C, st)
        else:
            self.fwd.add("mny_bn_eval_coeffs", gam, bet, rm, rv, BN_EPS, u.scale, u.shift, u.C, st)       # (st: an eval-mode unit of the dead branch stays on its stream)
            if self.frozen:                          # the backward kernels' yhat = (y - running_mean) * invstd
                self.fwd.add("mny_bn_eval_stats", rm, rv, BN_EPS, u.mean, u.invstd, u.C, st)
            # An eval-mode unit of a batch-statistics plan sits below the frontier (check_bn_modes) and has no backward call, so its
            # u.mean / u.invstd stay unwritten on purpose.  The only readers are the fused `_red` data-gradient kernels of the units right
            # above the frontier (mny_pw_bnbwd_red, mny_dw_bnbwd_red, mny_exdw_bwd_red, mny_pw_lr_fix), which form this unit's BN-backward
            # sums as a by-product: those sums are never consumed (no finalize runs for this unit), whatever they were computed from.

    def _emit_pw_gemm(self, calls, x, wop, w6, bias, addend, out, stats, M, K, Nc, st, tag=""):
        """out[M][Nc] = view(x)[M][K] . wop^T (+ bias) (+ addend): the pointwise forward GEMM, also the plain data gradient (x = dY, wop = W^T).
        w6: `wop` holds the pre-cut planes of the six-product bf16 form (_w6_planes)."""
        calls.add("mny_pw_fwd_w6" if w6 else self.K("mny_pw_fwd"), x[0], x[1], x[2], x[3], wop, bias, addend, out, stats, M, K, Nc, st,
                  label=self.K("mny_pw_fwd"),
                  meta=dict(flops=2 * M * K * Nc, bytes=self.eb * (M * K + M * Nc) + 4 * K * Nc, shape="%sM%d K%d N%d" % (tag, M, K, Nc)))

    def _fwd_weight(self, w, M, K, Nc):
        """-> (weight operand of a forward pointwise GEMM, whether it is the pre-cut six-product form)."""
        w6 = self._w6_planes(w, M, K, Nc)
        return (w6, True) if w6 is not None else (self._gemm_weight(w), False)

    def _fwd_unit(self, nd, st, sws):
        """stem / depthwise / pointwise conv + BatchNorm (+ activation, applied by the consumers' views)."""
        o = nd.out
        u = self._new_unit(o, materialise=o.id not in self.exdw_pw)      # the expand output of an exdw unit is never materialised
        stats = sws if self._batch_stats(nd.bn) else None
        if nd.op == "stem":
            conv = self._fwd_stem
        elif nd.op == "dw":
            conv = self._fwd_exdw_dw if o.id in self.exdw_dw else self._fwd_dw
        else:
            conv = self._fwd_exdw_pw if o.id in self.exdw_pw else self._fwd_pw
        parts = conv(nd, u, self._P[nd.conv + ".weight"], stats, st)
        self._emit_bn_tail(nd.bn, u, parts, u.M, sws, st)

    def _fwd_stem(self, nd, u, w, stats, st):
        N, H, W, C = self.N, self.H, self.W, u.C
        self.fwd.add(self.K("mny_stem_fwd"), self.x_ptr, w, u.Y, stats, N, H, W, C, self.stream,
                     meta=dict(flops=2 * u.M * C * 27, bytes=4 * N * 3 * H * W + self.eb * u.M * C))
        return _lib.query("mny_stem_stat_parts", N, H, W, C)

    def _fwd_exdw_dw(self, nd, u, w, stats, st):
        pn = self.exdw_dw[nd.out.id]                 # the expand node: x = its input (a view), e = its BN coefficients
        pi, pu = pn.ins[0], self.units[pn.out.id]
        psh = self._shape(pi)
        xv = self._view(pi)
        N, M, C = self.N, u.M, u.C
        Mx = N * psh[1] * psh[2]
        self.fwd.add("mny_exdw_fwd", xv[0], xv[1], xv[2], xv[3], self._P[pn.conv + ".weight"], pu.scale, pu.shift, w, u.Y, stats,
                     N, psh[1], psh[2], pi.C, C, 2, self.stream,
                     meta=dict(flops=2 * Mx * pi.C * C + 2 * M * C * 9, bytes=self.eb * (Mx * pi.C + M * C), shape="exdw K%d C%d H%d" % (pi.C, C, psh[1])))
        return _lib.query("mny_exdw_fwd_parts", N, psh[1], psh[2], pi.C, C, 2)

    def _fwd_dw(self, nd, u, w, stats, st):
        i = nd.ins[0]
        ish = self._shape(i)
        xv = self._view(i)
        N, M, C = self.N, u.M, u.C
        self.fwd.add(self.K("mny_dw_fwd"), xv[0], xv[1], xv[2], xv[3], w, u.Y, stats, N, ish[1], ish[2], C, nd.k, nd.stride, st,
                     meta=dict(flops=2 * M * C * nd.k * nd.k, bytes=self.eb * (N * ish[1] * ish[2] * C + M * C) + 4 * C * nd.k * nd.k,
                               shape="C%d H%d s%d" % (C, ish[1], nd.stride)))
        return _lib.query("mny_dw_stat_parts_x", N, ish[1], ish[2], C, nd.k, nd.stride, 1 if self.bf16 else 0)

    def _fwd_exdw_pw(self, nd, u, w, stats, st):
        i = nd.ins[0]
        xv = self._view(i)
        M, C = u.M, u.C
        if stats is not None:                        # batch statistics of the un-materialised expand output (eval plans / eval-mode units use the running ones)
            self.fwd.add("mny_exdw_stats", xv[0], xv[1], xv[2], xv[3], w, stats, M, i.C, C, self.stream,
                         meta=dict(flops=2 * M * i.C * (i.C + 1), bytes=self.eb * M * i.C,      # X^T X and colsum(X): one read of the thin X
                                   shape="exdw stats M%d K%d N%d" % (M, i.C, C)))
        return _lib.query("mny_exdw_stat_parts", M, i.C, C)

    def _fwd_pw(self, nd, u, w, stats, st):
        i = nd.ins[0]
        wop, w6 = self._fwd_weight(w, u.M, i.C, u.C)
        self._emit_pw_gemm(self.fwd, self._view(i), wop, w6, None, None, u.Y, stats, u.M, i.C, u.C, st)
        return _lib.query(self.K("mny_pw_stat_parts"), u.M, i.C, u.C)

    def _fwd_head(self, nd, st, sws):
        """`pwb`: a biased pointwise conv without BatchNorm (detection / segmentation head)."""
        o, i = nd.out, nd.ins[0]
        t = self._new_real(o)
        M = t.numel() // o.C
        wop, w6 = self._fwd_weight(self._P[nd.conv + ".weight"], M, i.C, o.C)
        self._emit_pw_gemm(self.fwd, self._view(i), wop, w6, self._P[nd.conv + ".bias"], None, t, None, M, i.C, o.C, st)
        if self.bf16:                    # loss / decode read the head in fp32
            t32 = torch.empty(t.shape, **self._f32)
            self.fwd.add("mny_cvt_bf16_f32", t, t32, t.numel(), st)
            self.head32[o.id] = t32
        g = self.net.graph
        if g.outputs and o is g.outputs[0]:
            self._head0_call = self.fwd.calls[-1]        # the first head exists behind THIS call (found again by identity: batched launches are inserted at the head of the list later)

    def _fwd_add(self, nd, st, sws):
        a = self._view(nd.ins[0])
        has_b, has_up = nd.k & 1, nd.k & 2
        b = self._view(nd.ins[1]) if has_b else _NO_VIEW
        up = self.reals[nd.ins[-1].id] if has_up else None
        if has_up:
            assert nd.ins[-1].kind == "real"
        t = self._new_real(nd.out)
        self.fwd.add(self.K("mny_add_views"), a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3], up, t, *t.shape, st)

    def _fwd_mul(self, nd, st, sws):
        a, b = self._view(nd.ins[0]), self._view(nd.ins[1])
        t = self._new_real(nd.out)
        self.fwd.add(self.K("mny_mul_views"), a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3], t, t.numel() // nd.out.C, nd.out.C, self.stream)

    def _fwd_partadd(self, nd, st, sws):
        a = self._view(nd.ins[0])
        up = self.reals[nd.ins[1].id]
        t = self._new_real(nd.out)
        self.fwd.add(self.K("mny_partadd_up"), a[0], a[1], a[2], a[3], up, t, t.shape[0], t.shape[1], t.shape[2], nd.ins[0].C, nd.out.C, st)

    _FWD = {"stem": _fwd_unit, "dw": _fwd_unit, "pw": _fwd_unit, "pwb": _fwd_head, "add": _fwd_add, "mul": _fwd_mul, "partadd": _fwd_partadd}

    def _emit_gate_forward(self, gate, nd):
        """The forward calls of a per-pixel gate (csrc/gate.hip) at node `nd` (the multiply, or the residual add that absorbs it)."""
        t, se0, se3 = gate["t"], gate["se0"], gate["se3"]
        u1, u2 = self.units[se0.out.id], self.units[se3.out.id]
        tsh = self._shape(t)
        M, C, R = tsh[0] * tsh[1] * tsh[2], t.C, se0.out.C
        tv = self._view(t)
        wq = gate["wq"]
        out = self._new_real(nd.out)
        parts = _lib.query("mny_gate_parts", M)
        eb = self.eb
        for un, hn in ((u1, se0), (u2, se3)):
            if self._batch_stats(hn.bn) and hn is se0:
                self.fwd.add("mny_gate_stats1_bf16", tv[0], tv[1], tv[2], wq, self.stats_ws, M, C, R, self.stream,
                             meta=dict(flops=2 * M * C * R, bytes=eb * M * C, shape="gate stats1 M%d C%d R%d" % (M, C, R)))
            elif self._batch_stats(hn.bn):
                self.fwd.add("mny_gate_stats2_bf16", tv[0], tv[1], tv[2], wq, u1.scale, u1.shift, self.stats_ws, M, C, R, self.stream,
                             meta=dict(flops=4 * M * C * R, bytes=eb * M * C, shape="gate stats2 M%d C%d R%d" % (M, C, R)))
            self._emit_bn_tail(hn.bn, un, parts, M, self.stats_ws, self.stream)
        a = _NO_VIEW
        if gate["add"] is not None:
            a = self._view(gate["add"].ins[1])
        self.fwd.add("mny_gate_fwd_bf16", tv[0], tv[1], tv[2], wq, u1.scale, u1.shift, u2.scale, u2.shift, a[0], a[1], a[2], a[3], out,
                     M, C, R, self.stream,
                     meta=dict(flops=4 * M * C * R, bytes=eb * M * C * (3 if a[0] is not None else 2), shape="gate M%d C%d R%d%s" % (M, C, R, " +add" if a[0] is not None else "")))

    def _flush_gate_jobs(self):
        """The gates' weights as matrix-core operand chunks, one launch per pass for all of them, at the head of the forward list."""
        if not self.gates:
            return
        P, gl = self._P, list(self.gates.values())
        rows = [(P[gt["se0"].conv + ".weight"].data_ptr(), P[gt["se3"].conv + ".weight"].data_ptr(), gt["wq"].data_ptr(), gt["t"].C, gt["se0"].out.C) for gt in gl]
        self.gate_jobs, _ = self._job_table(rows, [("w1", np.uint64), ("w2", np.uint64), ("wq", np.uint64), ("C", np.int32), ("R", np.int32)])
        self.fwd.add("mny_gate_cut_batch_bf16", self.gate_jobs, len(gl), self.stream)
        self.fwd.calls.insert(0, self.fwd.calls.pop())

    # ------------------------------------------------------------------------------------------
    def _build_detection(self):
        net, dev, N = self.net, self.dev, self.N
        f32 = dict(device=dev, dtype=torch.float32)
        self.hp, self.anchors, self.masks = [], [], []
        img = [self.H, self.W]                                  # mbv2_yolo.py:139-140 (Q8: [H,W] against (w,h) anchors)
        for hi, hs in enumerate(net.yolo_losses):
            g = self.heads[hi].shape[1]
            assert self.heads[hi].shape[1] == self.heads[hi].shape[2], "square grids only (yolo_loss.py:71)"
            hs.img_size = img
            anchors = torch.tensor([(aw / img[0], ah / img[1]) for aw, ah in hs.anchors], dtype=torch.float32).to(dev)
            self.anchors.append(anchors)
            self.masks.append(torch.tensor(hs.mask, dtype=torch.int32).to(dev))
            self.hp.append(YoloHead(N, g, len(hs.mask), hs.num_classes, len(hs.anchors), hs.ignore_threshold, hs.iou_thresh, hs.iou_weighting))
        if self.training:
            self.out14 = torch.zeros(2, 7, **f32)
            self.dheads = [torch.empty_like(h) for h in self.heads]
            self.t_ptr, self.off_ptr = _vp(0), _vp(0)
            self.loss_ws = []
            for hi in range(2):
                nbytes = _lib.query("mny_yolo_loss_ws_bytes", ctypes.byref(self.hp[hi]), 0)
                ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
                self.loss_ws.append(ws)
                # the first head's loss (five short, latency-bound launches) runs on the side stream from the moment that head exists, next to the
                # second head's branch (round 6; joined at the end of the list)
                pos = next((k + 1 for k, c in enumerate(self.fwd.calls) if c is self._head0_call), None)
                early = (hi == 0 and self.side_on and self.bn_batch and pos is not None and pos < len(self.fwd.calls))
                self.fwd.add("mny_yolo_loss", self.heads[hi], self.t_ptr, self.off_ptr, self.anchors[hi], self.masks[hi],
                             ctypes.byref(self.hp[hi]), self.out14[hi], self.dheads[hi], ws, self.stream_side if early else self.stream)
                if early:
                    loss_call = self.fwd.calls.pop()
                    self.fwd.add_py(self._fork_side, "fork")
                    fork_call = self.fwd.calls.pop()
                    self.fwd.calls[pos:pos] = [fork_call, loss_call]
                    self._loss_side = True
            self.t_dev = torch.zeros(max(4 * N, 64), 5, **f32)
            self.off_dev = torch.zeros(N + 1, device=dev, dtype=torch.int32)
            if self.seg_head is not None:             # mbv2_yolo.py:167-170: SegLoss on the raw seg head
                self.seg_out3 = torch.zeros(3, **f32)
                self.seg_maps = torch.zeros_like(self.seg_head)                 # resident copy of the batch's seg_maps [N,h,w,C]
                self.dheads.append(torch.empty_like(self.seg_head))
                self.seg_ws = torch.empty(max(_lib.query("mny_seg_loss_ws_bytes", self.seg_head.numel()), 8), device=dev, dtype=torch.uint8)
                self.fwd.add("mny_seg_loss", self.seg_head, self.seg_maps, self.seg_head.numel(), self.seg_out3, self.dheads[2], self.seg_ws, self.stream)
        else:
            C = net.num_classes
            self.cells = [hp.A * hp.g * hp.g for hp in self.hp]
            self.cap = sum(self.cells)
            self.rows = torch.zeros(N, self.cap, 7, **f32)
            self.cnt0 = torch.zeros(N, device=dev, dtype=torch.int32)
            self.cnt1 = torch.zeros(N, device=dev, dtype=torch.int32)
            self.seg_begin = (torch.arange(N, dtype=torch.int32) * self.cap).to(dev)
            self.out_idx = torch.zeros(N * self.cap, device=dev, dtype=torch.int32)
            self.out_counts = torch.zeros(N, device=dev, dtype=torch.int32)
            self.out_rows = torch.zeros(N * self.cap, 7, **f32)
            self.nms_ws = torch.empty(_lib.query("mny_nms_ws_bytes", N, N * self.cap, C), device=dev, dtype=torch.uint8)
            self.val_conf = [ctypes.c_float(0.1), ctypes.c_float(0.1)]
            self.det = CallList()
            self.det.add("mny_yolo_decode", self.heads[0], self.anchors[0], self.masks[0], ctypes.byref(self.hp[0]), self.val_conf[0],
                         self.rows, self.cap, None, self.cnt0, self.stream)
            self.det.add("mny_yolo_decode", self.heads[1], self.anchors[1], self.masks[1], ctypes.byref(self.hp[1]), self.val_conf[1],
                         self.rows, self.cap, self.cnt0, self.cnt1, self.stream)
            self.det_nms = len(self.det.calls)      # index of the NMS call (forward_eval(nms=False) steps over it)
            self.det.add("mny_nms_per_class", self.rows, self.seg_begin, self.cnt1, N, N * self.cap, self.cap, C, ctypes.c_double(0.45),
                         self.out_idx, self.out_counts, self.out_rows, self.nms_ws, self.stream)
            so = _lib.query("mny_nms_status_offset", N, N * self.cap, C)
            self.nms_status = self.nms_ws[so:so + 4].view(torch.int32)
            if self.seg_head is not None:             # mbv2_yolo.py:161-164 -> seg_loss.py:77-80: sigmoid of image 0, [C,h,w]
                _, sh, sw, sc = self.seg_head.shape
                self.seg_eval = torch.zeros(sc, sh, sw, **f32)
                self.det.add("mny_seg_sigmoid", self.seg_head, sh, sw, sc, self.seg_eval, self.stream)


    # ---- backward list ------------------------------------------------------------------------------
    def _build_backward(self, g):
        """State of the backward builder (all of it initialised here), the gradients of the loss inputs, then per node: the unit's emitter
        (_bwd_emitter) and the common tail."""
        bwd = self.bwd = CallList()
        fr = self.frontier
        order = fr.order             # == self.bwd_order with every parameter trainable; else cut at the frontier (frontier.py)
        self._plan_grad_arena(order)
        self._written = set()        # parameter names whose arena slot has its first contribution
        self.shared_tmp = []         # (scratch, arena view): later contributions of a module applied twice, added in by _flush_shared
        self._red_jobs, self._red_keep, self._post_reduce = [], [], []     # deferred partial combines (_defer_job / _flush_reduce)
        self._uses = {}              # conv name -> applications (a module applied twice, mbv3_yolo.py:133-134, adds a second contribution
        for nd in self.bwd_order:    # right after its producing call: its combines stay inline).  Counted over the whole graph, not the part
            if nd.conv:              # above the frontier: a unit that straddles it is emitted exactly as in the full plan, its unwanted
                self._uses[nd.conv] = self._uses.get(nd.conv, 0) + 1      # outputs (data gradient, BN sums of a frozen producer) landing in scratch
        self._frozen_scratch = []    # where the kernels above the frontier leave the gradients of frozen parameters (never exposed)
        self.fin_name = "mny_bn_bwd_finalize_frozen" if self.frozen else "mny_bn_bwd_finalize"
        self._gs = {v.id: _Grad() for v in g.values}
        self.grad_bufs = []
        self.fused_red = {}      # value id -> (partial-sum buffer, rows) written by the data-gradient GEMM that produced the value's gradient
        self.stemdw_done = set() # stem output ids whose whole backward (BN sums, weight gradient) left with the depthwise consumer's (mny_stemdw_bwd)
        # wide expand units on the low-rank BN backward (csrc/lrbwd.hip): the depthwise unit behind stores ca o G o act'(z), both GEMMs run on
        # that tensor and the BatchNorm terms are K-wide corrections — no bn_bwd_apply pass over the C-wide tensors.  lr_units: value ids
        self.lr_units = set()
        self._alloc_bwd_workspaces(g, order)
        self._seed_loss_grads()
        self._emit_weight_transposes(order)
        for nd in order:
            o = nd.out
            if o.id in self.exdw_pw or o.id in self.stemdw_done:
                continue                                   # handled with its depthwise consumer (mny_exdw_bwd / mny_stemdw_bwd)
            if o.id in self.gate_units or o.id in self.gate_absorbed:
                continue                                   # hidden units / absorbed multiply of a per-pixel gate: handled where the gate was emitted
            G = self._gs[o.id].buf
            assert G is not None, "no gradient reached %s" % o.name
            self._bwd_emitter(nd)(nd, G)
            self._flush_shared()
            self._flush_reduce()
            bwd.marks[o.name] = len(bwd.calls)
        self._flush_reduce(force=True)

    def _plan_grad_arena(self, order):
        """Flat gradient arena in backward production order (heads first -> DP buckets complete early)."""
        P = self._P
        self.grad_params = []
        off = 0
        slots = {}
        # detection heads: dL/dhead rows are padded to `head_cp` channels for the backward GEMMs (mny_pad_rows); the pad rows of
        # dW / pad entries of dbias land in slack reserved behind the parameter's gradient slot
        align = 8 if self.bf16 else 4
        self.head_cp = {nd.out.id: (nd.out.C + align - 1) // align * align for nd in order
                        if nd.op == "pwb" and nd.out.C % align}
        slack = {}
        for nd in order:
            if nd.out.id in self.head_cp:
                cp = self.head_cp[nd.out.id]
                slack[nd.conv + ".weight"] = cp * nd.ins[0].C
                slack[nd.conv + ".bias"] = cp
        for nd in order:
            for nm in frontier.node_params(nd):
                if nm in slots or nm in self.frontier.frozen:
                    continue                     # module applied twice (mbv3_yolo.py:133-134): one slot, two contributions; a frozen parameter: none
                n = P[nm].numel()
                slots[nm] = (off, n)
                self.grad_params.append(nm)
                off += (max(n, slack.get(nm, 0)) + 3) // 4 * 4
        assert self.grad_params == self.frontier.grad_params
        self._slack = slack
        self.gflat = torch.zeros(off, **self._f32)
        self.gviews = {nm: self.gflat[o:o + n].view(P[nm].shape) for nm, (o, n) in slots.items()}
        self.grad_slots = slots

    def _alloc_bwd_workspaces(self, g, order):
        """Workspaces shared by all layers (single stream => sequential use)."""
        ws_floats = 1
        for nd in order:
            o = nd.out
            M = self._rows(o)
            if nd.op in ("pw", "pwb"):
                ws_floats = max(ws_floats, _lib.query("mny_pw_wgrad_ws_floats", M, nd.ins[0].C, self.head_cp.get(o.id, o.C)),
                                _lib.query("mny_pw_bnbwd_ws_floats", M, nd.ins[0].C, o.C))
            elif nd.op == "dw":
                ws_floats = max(ws_floats, self.max_parts * o.C * nd.k * nd.k)     # (max_parts = 1024 >= the 768-row grids of the fused kernels)
            elif nd.op == "stem":
                ws_floats = max(ws_floats, self.max_parts * o.C * 27)
        self.ws = torch.empty(ws_floats, **self._f32)
        self.ws_side = torch.empty(ws_floats, **self._f32) if self.side_on else self.ws
        self.red_ws = torch.empty(2048 * 2 * self.maxC, **self._f32)      # >= mny_bn_bwd_parts() rows of [2][C]
        self.coef_ws = torch.empty(3 * self.maxC, **self._f32)
        self.g_scale = torch.ones(len(self.loss_outputs), **self._f32)   # upstream dL/dloss_i, written by backward()

    def _seed_loss_grads(self):
        """dL/d(loss input) = upstream scale * what the loss call left, padded for the heads whose channel count the GEMMs cannot take."""
        bwd, gs = self.bwd, self._gs
        for hi, o in enumerate(self.loss_outputs):
            if not self.frontier.needs_grad(o):
                continue                     # nothing trainable feeds this loss
            dh = self.dheads[hi]
            if o.id in self.head_cp:
                cp = self.head_cp[o.id]
                shp = self._shape(o)
                gp = torch.empty(shp[0], shp[1], shp[2], cp, **self._act)
                bwd.add(self.K("mny_pad_rows"), dh, self.g_scale[hi:hi + 1], gp, self._rows(o), o.C, cp, self.stream)
                gs[o.id].buf = gp
                continue
            bwd.add("mny_axpy", dh, self.g_scale[hi:hi + 1], dh, 0, dh.numel(), self.stream)
            if self.bf16:
                d16 = torch.empty(dh.shape, **self._act)
                bwd.add("mny_cvt_f32_bf16", dh, d16, d16.numel(), self.stream)
                gs[o.id].buf = d16
            else:
                gs[o.id].buf = dh

    def _emit_weight_transposes(self, order):
        """W^T of every generic pointwise unit, all in one launch at the head of the backward list (one per layer was 39 launches)."""
        rows, block_job = [], []
        for nd in order:
            if nd.op not in ("pw", "pwb") or self._takes_own_sums(nd) or nd.conv in self.wT:
                continue
            if not self.frontier.needs_grad(nd.ins[0]) and not self._lr_ok(nd):
                continue                     # at the frontier: the generic route leaves the data gradient out (the low-rank route runs whole)
            w = self._P[nd.conv + ".weight"]
            oc = self.head_cp.get(nd.out.id, nd.out.C)
            wT = torch.empty(nd.ins[0].C, oc, **self._act)
            self.wT[nd.conv] = wT
            rows.append((w.data_ptr(), wT.data_ptr(), nd.out.C, nd.ins[0].C, oc, len(block_job)))
            block_job += [len(rows) - 1] * (((nd.ins[0].C + 31) // 32) * ((oc + 31) // 32))
        if not rows:
            return
        self.t_jobs, self.t_blocks = self._job_table(rows, [("src", np.uint64), ("dst", np.uint64), ("R", np.int32), ("Cc", np.int32), ("Rp", np.int32), ("b0", np.int32)], block_job)
        self.bwd.add(self.K("mny_transpose_batch"), self.t_jobs, self.t_blocks, len(block_job), self.stream)
        # ... and, for the data-gradient GEMMs that take the six-product bf16 form, the cut of W^T right behind it
        for nd in order:
            if nd.conv in self.wT and nd.conv not in self.wT6 and not self._takes_own_sums(nd):
                oc = self.head_cp.get(nd.out.id, nd.out.C)
                pl6 = self._w6_planes(self.wT[nd.conv], self._rows(nd.out), oc, nd.ins[0].C)
                if pl6 is not None:
                    self.wT6[nd.conv] = pl6
        self._flush_cut_jobs(self.bwd)

    # ---- backward: steps shared by the emitters ----------------------------------------------------
    def _single(self, nd):
        return self._uses.get(nd.conv, 0) == 1

    def _gv(self, nm):
        """Destination of a parameter gradient.  The first contribution writes the arena slot; a later one (shared
        module) writes a scratch tensor that `_flush_shared()` adds into the slot right after the producing call."""
        if nm in self.frontier.frozen:       # frozen parameter above the frontier: the kernels run as they do, into scratch
            p = self._P[nm]
            buf = torch.empty(max(p.numel(), self._slack.get(nm, 0)), **self._f32)
            self._frozen_scratch.append(buf)
            return buf[:p.numel()].view(p.shape)
        if nm not in self._written:
            self._written.add(nm)
            return self.gviews[nm]
        tmp = torch.empty_like(self.gviews[nm])
        self.shared_tmp.append((tmp, self.gviews[nm]))
        return tmp

    def _flush_shared(self):
        while self.shared_tmp:
            tmp, dst = self.shared_tmp.pop()
            self.bwd.add("mny_axpy", tmp, None, dst, 1, tmp.numel(), self.stream)

    # Deferred partial combines: every weight-gradient call leaves per-workgroup partial sums; instead of one small combine
    # launch per layer (70 launches of 8-10 us at bs=256, 0.66 ms/step) the layer gets its OWN partial buffer, is called with
    # dw = NULL, and a whole run of layers is combined by one mny_reduce_batch launch (_flush_reduce: every DEFER_EVERY jobs, so
    # the data-parallel buckets still complete early).
    DEFER_EVERY = 16

    def _defer_job(self, n_floats, dest, nparts, n):
        """-> private partial buffer of a deferred combine writing `dest` (an arena view)."""
        wsl = torch.empty(max(int(n_floats), 1), **self._f32)
        self._red_jobs.append((wsl, dest, int(nparts), int(n)))
        return wsl

    def _wgrad_dest(self, nd, parts, n, shared_ws, floats=None, also=True):
        """-> (dw, ws) arguments of a weight-gradient kernel leaving `parts` partial rows of `n` floats: (None, a private partial buffer
        combined later) for a module applied once, else (the arena view or scratch, the shared workspace) with the combine inline.
        `parts` may be a callable (asked only when the job is deferred); floats(parts): size of the private buffer if not parts * n."""
        dwv = self._gv(nd.conv + ".weight")
        if not (also and self._single(nd)):
            return dwv, shared_ws
        p = parts() if callable(parts) else parts
        return None, self._defer_job(floats(p) if floats else p * n, dwv, p, n)

    def _flush_reduce(self, force=False):
        if not self._red_jobs or (not force and len(self._red_jobs) < self.DEFER_EVERY):
            return
        bwd = self.bwd
        rows, block_job = [], []
        for wsl, dest, nparts, n in self._red_jobs:
            rows.append((wsl.data_ptr(), dest.data_ptr(), n, nparts, len(block_job)))
            block_job += [len(rows) - 1] * ((n + 31) // 32)
        jdev, bdev = self._job_table(rows, [("parts", np.uint64), ("out", np.uint64), ("n", np.int64), ("nparts", np.int32), ("b0", np.int32)], block_job)
        self._red_keep += [t for job in self._red_jobs for t in job[:2]]
        # The combine feeds nothing downstream in the backward pass: it runs on the SIDE stream, behind the side-stream weight gradients
        # whose partial rows it reads (same stream = ordered) and, through the fork, behind everything the main stream has enqueued (the
        # fused units leave their partial rows there).  Every replayed segment ends with a join (run_bwd_segment), so gradients are
        # complete before an all-reduce or the optimizer sees them.  (Round 4 joined here and ran the combine on the main stream: 0.3 ms
        # of 4-5 launches on the critical path of both benchmark configurations.)
        if self.side_on:
            bwd.add_py(self._fork_side, "fork")
            red_stream = self.stream_side
        else:
            red_stream = self.stream
        bwd.add("mny_reduce_batch", jdev, bdev, len(block_job), red_stream, meta=dict(writes=[job[1].data_ptr() for job in self._red_jobs]))
        for hook in self._post_reduce:                        # corrections of combined weight gradients (low-rank BN backward): same stream, right behind the combine
            hook(red_stream)
        self._red_jobs, self._post_reduce = [], []

    def _alloc_grad(self, v):
        t = torch.empty(self._shape(v), **self._act)
        self.grad_bufs.append(t)
        return t

    def _accumulate_into(self, v, emit):
        """emit(dst, accumulate) appends a call that writes (accumulate = 0) or adds to (1) the gradient of `v`, whose buffer is made
        private first if it is an alias of another value's."""
        s = self._gs[v.id]
        if s.buf is None:
            s.buf, s.shared = self._alloc_grad(v), False
            emit(s.buf, 0)
            return
        if s.shared:
            nb = self._alloc_grad(v)
            self.bwd.add(self.K("mny_axpy"), s.buf, None, nb, 0, nb.numel(), self.stream)
            s.buf, s.shared = nb, False
        emit(s.buf, 1)

    def _contribute_alias(self, v, buf):
        s = self._gs[v.id]
        if s.buf is None:
            s.buf, s.shared = buf, True
        else:
            self._accumulate_into(v, lambda dst, acc: self.bwd.add(self.K("mny_axpy"), buf, None, dst, acc, dst.numel(), self.stream))

    def _contribute_kernel(self, v, emit, inplace_ok=True):
        """emit(out, addend) appends the producing call.  inplace_ok=False: the kernel cannot take addend == out (the two-pass
        expand + depthwise backward overwrites `out` before it reads the addend): an existing gradient becomes the addend of a fresh buffer."""
        s = self._gs[v.id]
        if s.buf is None:
            s.buf, s.shared = self._alloc_grad(v), False
            emit(s.buf, None)
        elif not s.shared and inplace_ok:
            emit(s.buf, s.buf)
        else:
            nb = self._alloc_grad(v)
            emit(nb, s.buf)
            s.buf, s.shared = nb, False

    def _bn_sums(self, nd, G):
        """The BN-backward preamble of a unit: the sums that left with the producer of G, else mny_bn_bwd_reduce; then the finalize
        (dgamma, dbeta, and the unit's coefficients into coef_ws)."""
        o, u = nd.out, self.units[nd.out.id]
        red_buf, red_parts = self.fused_red.get(o.id, (None, 0))
        if red_buf is None:
            red_buf, red_parts = self.red_ws, _lib.query("mny_bn_bwd_parts", u.M, o.C)
            self.bwd.add(self.K("mny_bn_bwd_reduce"), G, u.Y, u.scale, u.shift, o.act, u.mean, u.invstd, self.red_ws, u.M, o.C, self.stream,
                         meta=dict(flops=0, bytes=2 * self.eb * u.M * o.C, shape="M%d C%d" % (u.M, o.C)))
        self.bwd.add(self.fin_name, red_buf, red_parts, u.M, self._P[nd.bn + ".weight"], u.mean, u.invstd, self._gv(nd.bn + ".weight"), self._gv(nd.bn + ".bias"),
                     self.coef_ws, o.C, self.stream)

    def _takes_own_sums(self, pn):
        """True for the thin expand units handled by mny_pw_bnbwd (their stage 1 forms the BN sums itself)."""
        if pn.op != "pw" or self.frozen:
            return False                     # (frozen BatchNorm: that unit's own finalize assumes batch statistics)
        po, pi = pn.out, pn.ins[0]
        if pi.act in _HARD or po.act in _HARD:
            return False
        return _lib.query(self.K("mny_pw_bnbwd_supported"), self._rows(po), pi.C, po.C) == 1

    def _sole_producer(self, i, xv, ops, no_acts=(), need_single=False, own_sums_ok=False):
        """Is the input `i` (seen as the view `xv`) the raw output of a conv+BN+act unit of kind `ops` that only the node being emitted
        consumes and that has no gradient yet?  Then the data gradient about to be written is that unit's COMPLETE output gradient and its
        BN-backward sums can leave with it.  no_acts: activations of `i` the fused kernel does not take; need_single: the producer's module
        must be applied once; own_sums_ok: do not ask whether the producer forms its own sums (_takes_own_sums)."""
        prod = i.node
        return (i.kind == "unit" and prod is not None and prod.op in ops and self._gs[i.id].buf is None and self.n_consumers[i.id] == 1
                and (own_sums_ok or not self._takes_own_sums(prod)) and xv[1] is not None and i.act not in no_acts
                and (not need_single or self._single(prod)))

    def _new_fused_red(self, v, parts):
        """-> partial-sum buffer ([parts][2][C]) that a data-gradient kernel fills with the BN-backward sums of the unit `v` (read by _bn_sums)."""
        rbuf = torch.empty(parts * 2 * v.C, **self._f32)
        self.fused_red[v.id] = (rbuf, parts)
        return rbuf

    def _red_target(self, i, nd):
        """The conv+BN+act unit whose COMPLETE output gradient the data gradient of `nd` w.r.t. its input `i` is — its BN-backward sums can
        leave with that gradient (no mny_bn_bwd_reduce pass) — or None.  `i` itself when it is a unit and `nd` its last consumer; or, looking
        through a residual add (round 6): the add's unit operand that only the add consumes takes the sum's gradient unchanged (an alias)."""
        if i.id in self.out_ids or self.last_consumer.get(i.id) is not nd:
            return None
        t = None
        if i.kind == "unit":
            t = i
        elif i.node is not None and i.node.op == "add":
            cands = [v for v in i.node.ins[:1 + (i.node.k & 1)] if v.kind == "unit" and self.n_consumers[v.id] == 1 and v.id not in self.out_ids]
            if len(cands) == 1:
                t = cands[0]
        if (t is None or t.node is None or t.node.op not in ("dw", "pw") or self._takes_own_sums(t.node) or t.id not in self.units
                or self.units[t.id].Y is None or self._gs[t.id].buf is not None and t is not i):
            return None
        return t

    def _lr_ok(self, pn):
        if (self.bf16 or self.frozen or pn.op != "pw" or pn.bias or not self._single(pn) or pn.out.id in self.head_cp
                or self._takes_own_sums(pn) or self.sw_no_lr):
            return False
        pi = pn.ins[0]
        if pi.act != ACT_NONE or pi.kind not in ("unit", "real"):
            return False                     # the thin input's view must be linear: it is folded into the correction's operands
        return _lib.query("mny_lr_supported", self._rows(pn.out), pi.C, pn.out.C) == 1

    # ---- backward: one emitter per unit kind -------------------------------------------------------
    def _bwd_emitter(self, nd):
        """The method that emits the backward calls of `nd`, given the state of the list so far."""
        o = nd.out
        if o.id in self.gates:
            return self._bwd_gate
        if nd.op == "dw" and o.id in self.exdw_dw:
            return self._bwd_exdw
        if nd.op in ("add", "mul", "partadd"):
            return {"add": self._bwd_add, "mul": self._bwd_mul, "partadd": self._bwd_partadd}[nd.op]
        if nd.op == "pw" and self._takes_own_sums(nd):
            return self._bwd_thin_expand
        if nd.op == "pw" and o.id in self.lr_units:
            return self._bwd_lr_expand
        if nd.op == "dw" and o.act != _lib.ACT_HSIGMOID and nd.ins[0].act != _lib.ACT_HSIGMOID:
            if _lib.query("mny_dw_bnbwd_supported", nd.k, nd.stride) == 1:
                return self._bwd_dw_s1
            if nd.k == 3 and nd.stride == 2:
                return self._bwd_dw_s2
            if nd.k == 5 and nd.stride == 2 and not self.sw_no_dwfuse5s2 and o.C % 2 == 0:
                return self._bwd_dw_s2k5
        if self._project_ok(nd):
            return self._bwd_project
        return self._bwd_generic

    def _bwd_gate(self, nd, G):
        """per-pixel gate as one unit (csrc/gate.hip): three passes over (y3, dL/d out) with the two BN-backward finalizes in between; the
        hidden tensors' gradients are never written.  The residual operand (absorbed add) takes G itself."""
        bwd, P, gv, eb, gs = self.bwd, self._P, self._gv, self.eb, self._gs
        gate = self.gates[nd.out.id]
        t, se0, se3 = gate["t"], gate["se0"], gate["se3"]
        if gate["add"] is not None:
            self._contribute_alias(gate["add"].ins[1], G)
        u1, u2, u3 = self.units[se0.out.id], self.units[se3.out.id], self.units[t.id]
        tv = self._view(t)
        M, C, R = self._rows(nd.out), t.C, se0.out.C
        wq = gate["wq"]
        gparts = _lib.query("mny_gate_bwd_parts", M)
        coef2, coef1 = torch.empty(3 * C, **self._f32), torch.empty(3 * R, **self._f32)
        gate["coef"] = (coef2, coef1)
        bwd.add("mny_gate_bwd1_bf16", tv[0], tv[1], tv[2], G, wq, u1.scale, u1.shift, u2.scale, u2.shift, u2.mean, u2.invstd, self.red_ws, M, C, R, self.stream,
                meta=dict(flops=4 * M * C * R, bytes=eb * 2 * M * C, shape="gate bwd1 M%d C%d R%d" % (M, C, R)))
        bwd.add(self.fin_name, self.red_ws, gparts, M, P[se3.bn + ".weight"], u2.mean, u2.invstd, gv(se3.bn + ".weight"), gv(se3.bn + ".bias"), coef2, C, self.stream)
        ws2 = self._defer_job(gparts * C * R, gv(se3.conv + ".weight"), gparts, C * R)
        bwd.add("mny_gate_bwd2_bf16", tv[0], tv[1], tv[2], G, wq, u1.scale, u1.shift, u1.mean, u1.invstd, u2.scale, u2.shift, coef2, self.red_ws, ws2,
                M, C, R, self.stream, meta=dict(flops=8 * M * C * R, bytes=eb * 2 * M * C, shape="gate bwd2 M%d C%d R%d" % (M, C, R)))
        bwd.add(self.fin_name, self.red_ws, gparts, M, P[se0.bn + ".weight"], u1.mean, u1.invstd, gv(se0.bn + ".weight"), gv(se0.bn + ".bias"), coef1, R, self.stream)
        ws1 = self._defer_job(gparts * C * R, gv(se0.conv + ".weight"), gparts, C * R)
        rbuf = None
        prod = t.node
        if (_lib.query("mny_gate_bwd_red3_supported", C, R) == 1 and prod is not None and prod.op == "pw" and not self._takes_own_sums(prod)):
            rbuf = self._new_fused_red(t, gparts)                # dt is the project unit's complete output gradient: its BN-backward sums leave with it
        assert gs[t.id].buf is None, "the gate's input has another consumer"
        gs[t.id].buf, gs[t.id].shared = self._alloc_grad(t), False
        bwd.add("mny_gate_bwd3_bf16", tv[0], tv[1], tv[2], G, wq, u1.scale, u1.shift, u2.scale, u2.shift, coef2, coef1, u3.mean, u3.invstd, gs[t.id].buf, ws1, rbuf,
                M, C, R, self.stream, meta=dict(flops=12 * M * C * R, bytes=eb * 3 * M * C, shape="gate bwd3 M%d C%d R%d" % (M, C, R)))

    def _bwd_exdw(self, nd, G):
        """expand + depthwise unit: the depthwise unit's BN-backward sums as usual, then ONE entry point yields the depthwise and the
        expand unit's parameter gradients and the data gradient wrt the thin input; neither the expand output nor its gradient exists."""
        P, gv, N = self._P, self._gv, self.N
        o, u = nd.out, self.units[nd.out.id]
        pn = self.exdw_dw[o.id]
        pi, pu = pn.ins[0], self.units[pn.out.id]
        psh = self._shape(pi)
        xv = self._view(pi)
        geom = (N, psh[1], psh[2], pi.C, o.C, 2)
        self._bn_sums(nd, G)
        dparts = _lib.query("mny_exdw_bwd_parts", *geom)
        dwv_k, dws_k = self._wgrad_dest(nd, dparts, o.C * 9, None)
        if dws_k is None:
            dws_k = torch.empty(dparts * o.C * 9, **self._f32)
        xws = torch.empty(max(int(_lib.query("mny_exdw_bwd_ws_floats", *geom)), 4), **self._f32)
        dwe, dge, dbe = gv(pn.conv + ".weight"), gv(pn.bn + ".weight"), gv(pn.bn + ".bias")
        M, Mx, Kc, C = u.M, N * psh[1] * psh[2], pi.C, o.C
        # algorithmic: the expand output once per pass + P1 + dX; the transposed stencil per pass + dW_dw; X twice + dX once, G_z and Z twice
        meta = dict(flops=6 * Mx * Kc * C + 6 * M * C * 9, bytes=self.eb * (3 * Mx * Kc + 4 * M * C), shape="exdw K%d C%d H%d" % (Kc, C, psh[1]))
        # the thin input is the raw output of a conv+BN unit consumed only here (the project conv in front of the first expand unit):
        # the finished dX is that unit's complete output gradient -> its BN-backward sums leave with it, no separate reduce pass
        with_red = (self._sole_producer(pi, xv, ("pw", "dw", "stem"), no_acts=_HARD) and _lib.query("mny_exdw_bwd_red_parts", *geom) > 0)
        if with_red:
            ppu = self.units[pi.id]
            rbuf = self._new_fused_red(pi, _lib.query("mny_exdw_bwd_red_parts", *geom))
            meta["shape"] += " +red"

        def emit(out, addend):
            head = (G, u.Y, u.scale, u.shift, o.act, self.coef_ws, xv[0], xv[1], xv[2], xv[3])
            tail = (P[pn.conv + ".weight"], pu.scale, pu.shift, pu.mean, pu.invstd, P[pn.bn + ".weight"], P[nd.conv + ".weight"], addend, out,
                    dwe, dge, dbe, dwv_k, dws_k, xws)
            if with_red:
                self.bwd.add("mny_exdw_bwd_red", *head, ppu.mean, ppu.invstd, *tail, rbuf, *geom, self.stream, label="mny_exdw_bwd", meta=meta)
            else:
                self.bwd.add("mny_exdw_bwd", *head, *tail, *geom, self.stream, meta=meta)
        self._contribute_kernel(pi, emit, inplace_ok=False)

    def _bwd_add(self, nd, G):
        need = self.frontier.needs_grad
        if need(nd.ins[0]):
            self._contribute_alias(nd.ins[0], G)
        if nd.k & 1 and need(nd.ins[1]):
            self._contribute_alias(nd.ins[1], G)
        if nd.k & 2 and need(nd.ins[-1]):
            self._accumulate_into(nd.ins[-1], lambda dst, acc: self.bwd.add(self.K("mny_upsample_bwd"), G, dst, acc, *self._shape(nd.out), self.stream))

    def _bwd_mul(self, nd, G):
        M, C = self._rows(nd.out), nd.out.C
        va, vb = self._view(nd.ins[0]), self._view(nd.ins[1])

        def times(other):
            return lambda out, addend: self.bwd.add(self.K("mny_mul_views_bwd"), G, other[0], other[1], other[2], other[3], addend, out, M, C, self.stream)
        if self.frontier.needs_grad(nd.ins[0]):
            self._contribute_kernel(nd.ins[0], times(vb))
        if self.frontier.needs_grad(nd.ins[1]):
            self._contribute_kernel(nd.ins[1], times(va))

    def _bwd_partadd(self, nd, G):
        av, upv = nd.ins[0], nd.ins[1]
        M = self._rows(nd.out)
        if self.frontier.needs_grad(av):
            self._accumulate_into(av, lambda dst, acc: self.bwd.add(self.K("mny_slice_channels"), G, dst, acc, M, av.C, nd.out.C, self.stream))
        if self.frontier.needs_grad(upv):
            self._accumulate_into(upv, lambda dst, acc: self.bwd.add(self.K("mny_upsample_bwd"), G, dst, acc, *self._shape(nd.out), self.stream))

    def _bwd_thin_expand(self, nd, G):
        """thin "expand" unit: BN-backward + wgrad + dgrad from (G, Y, X) in 4 passes, dY never materialised."""
        P, gv = self._P, self._gv
        o, u, i = nd.out, self.units[nd.out.id], nd.ins[0]
        M, Kc, Nc = u.M, i.C, o.C
        xv = self._view(i)
        dwv, dgv, dbv = gv(nd.conv + ".weight"), gv(nd.bn + ".weight"), gv(nd.bn + ".bias")
        args = (G, u.Y, u.scale, u.shift, o.act, u.mean, u.invstd, P[nd.bn + ".weight"], xv[0], xv[1], xv[2], xv[3], P[nd.conv + ".weight"])
        # algorithmic: G, Y (stage 1) + G (stage 2); X twice, dX once
        meta = dict(flops=6 * M * Kc * Nc, bytes=self.eb * (3 * M * Nc + 3 * M * Kc), shape="M%d K%d N%d" % (M, Kc, Nc))
        # the data gradient of this unit completes the output gradient of the unit in front (the previous block's project conv, directly or
        # through the residual add): that unit's BN-backward sums leave with stage 2 (round 6: mny_pw_bnbwd_red, fp32 storage)
        tgt = self._red_target(i, nd) if not self.bf16 else None
        if tgt is not None and (tgt.act in _HARD or _lib.query("mny_pw_bnbwd_red_supported", M, Kc, Nc) != 1):
            tgt = None
        if tgt is not None:
            pu = self.units[tgt.id]
            assert tgt.C == Kc
            rbuf = self._new_fused_red(tgt, _lib.query("mny_pw_bnbwd_red_parts", M, Kc, Nc))
            meta["shape"] += " +red"
            self._contribute_kernel(i, lambda out, addend: self.bwd.add(
                "mny_pw_bnbwd_red", *args, addend, out, dwv, dgv, dbv, self.ws, pu.Y, pu.scale, pu.shift, tgt.act, pu.mean, pu.invstd, rbuf, M, Kc, Nc, self.stream,
                label="mny_pw_bnbwd", meta=meta))
        else:
            self._contribute_kernel(i, lambda out, addend: self.bwd.add(
                self.K("mny_pw_bnbwd"), *args, addend, out, dwv, dgv, dbv, self.ws, M, Kc, Nc, self.stream, meta=meta))

    def _bwd_lr_expand(self, nd, G):
        """wide expand unit, low-rank BN backward: G holds dzc = ca o dL/da o act'(z) (written by the depthwise unit behind, whose epilogue also
        left this unit's BN-backward sums).  dW = dzc^T X + cb o (W X^T X) + cc (x) colsum(X);  dX = dzc W + X Q + r."""
        bwd, gv, eb, f32 = self.bwd, self._gv, self.eb, self._f32
        o, u, i = nd.out, self.units[nd.out.id], nd.ins[0]
        xv = self._view(i)
        M, Kc, C = u.M, i.C, o.C
        w = self._P[nd.conv + ".weight"]
        red_buf, red_parts = self.fused_red[o.id]
        coef_u = torch.empty(3 * C, **f32)                 # private: the side-stream weight-gradient correction reads it long after coef_ws is reused
        bwd.add(self.fin_name, red_buf, red_parts, M, self._P[nd.bn + ".weight"], u.mean, u.invstd, gv(nd.bn + ".weight"), gv(nd.bn + ".bias"), coef_u, C, self.stream)
        bq, rb = torch.empty(Kc * Kc, **f32), torch.empty(Kc, **f32)
        prep_side = self.side_on       # Q, r under the main-term GEMM below; joined in front of the correction
        if prep_side:
            bwd.add_py(self._fork_side2, "fork")
        bwd.add("mny_lr_prep", coef_u, w, bq, rb, C, Kc, self.stream_side2 if prep_side else self.stream)
        dwv = gv(nd.conv + ".weight")
        if self.side_on:
            bwd.add_py(self._fork_side, "fork")
        st_w = self.stream_side if self.side_on else self.stream
        psplits = _lib.query("mny_pw_wgrad_splits", M, Kc, C)
        pws = self._defer_job(max(_lib.query("mny_pw_wgrad_ws_floats", M, Kc, C), psplits * C * Kc), dwv, psplits, C * Kc)
        bwd.add("mny_pw_wgrad", xv[0], xv[1], xv[2], xv[3], G, None, None, pws, M, Kc, C, st_w,
                meta=dict(flops=2 * M * Kc * C, bytes=eb * (M * Kc + M * C) + 4 * Kc * C, shape="M%d K%d N%d" % (M, Kc, C)))
        gparts = _lib.query("mny_lr_gram_parts", M, Kc)
        gsum = torch.empty(Kc * Kc + Kc, **f32)
        gws = self._defer_job(gparts * (Kc * Kc + Kc), gsum, gparts, Kc * Kc + Kc)
        bwd.add("mny_lr_gram", xv[0], xv[1], xv[2], xv[3], gws, M, Kc, st_w,
                meta=dict(flops=2 * M * Kc * Kc, bytes=eb * M * Kc, shape="gram M%d K%d" % (M, Kc)))
        self._post_reduce.append(lambda st: bwd.add("mny_lr_wfix", dwv, gsum, coef_u, w, C, Kc, st))
        wT6 = self.wT6.get(nd.conv)
        wop = wT6 if wT6 is not None else self.wT[nd.conv]
        self._contribute_kernel(i, lambda out, addend: self._emit_pw_gemm(
            bwd, (G, None, None, ACT_NONE), wop, wT6 is not None, None, addend, out, None, M, C, Kc, self.stream, tag="dgrad "))
        buf = self._gs[i.id].buf
        if prep_side:
            bwd.add_py(self._join_side2, "join")
        tgt = self._red_target(i, nd)
        if tgt is not None:
            pu = self.units[tgt.id]
            assert tgt.C == Kc
            rbuf = self._new_fused_red(tgt, _lib.query("mny_pw_lr_fix_parts", M, Kc, tgt.act))
            bwd.add("mny_pw_lr_fix", xv[0], xv[1], xv[2], bq, rb, buf, buf, pu.Y, pu.scale, pu.shift, tgt.act, pu.mean, pu.invstd, rbuf, M, Kc, self.stream,
                    meta=dict(flops=2 * M * Kc * Kc, bytes=eb * 4 * M * Kc, shape="lr fix+red M%d K%d" % (M, Kc)))
        else:
            bwd.add("mny_pw_lr_fix", xv[0], xv[1], xv[2], bq, rb, buf, buf, None, None, None, 0, None, None, None, M, Kc, self.stream,
                    meta=dict(flops=2 * M * Kc * Kc, bytes=eb * 3 * M * Kc, shape="lr fix M%d K%d" % (M, Kc)))

    def _bwd_dw_s1(self, nd, G):
        """3x3 (register form) / 5x5 (tile form, csrc/dwtile.hip) stride-1 depthwise unit: dY is rebuilt on chip, one pass over
        (G, Y, X) yields dX and dW."""
        P, gv, N = self._P, self._gv, self.N
        o, u, i = nd.out, self.units[nd.out.id], nd.ins[0]
        M, C, k, kk = u.M, o.C, nd.k, nd.k * nd.k
        ish = self._shape(i)
        xv = self._view(i)
        self._bn_sums(nd, G)
        wt = P[nd.conv + ".weight"]
        prod = i.node
        # the input is the raw output of a conv+BN+act unit consumed ONLY here: this kernel's dX is that unit's complete
        # output gradient, so it also leaves the unit's BN-backward sums (mny_dw_bnbwd_red) and the unit's separate
        # bn_bwd_reduce pass — a re-read of dX and X — disappears (wide expand units, the stem, the neck's pointwise units)
        with_red = self._sole_producer(i, xv, ("pw", "stem"), no_acts=(_lib.ACT_HSIGMOID,))
        pflags = (1 if self.bf16 else 0) | (2 if with_red else 0)        # (the row count depends on the form that runs: csrc/dwtile.hip dwt_use)
        dwv_k, ws_k = self._wgrad_dest(nd, lambda: _lib.query("mny_dw_bnbwd_parts_k", N, ish[1], ish[2], C, k, pflags), C * kk, self.ws)
        # stem -> this depthwise unit (MobileNetV2's first two units): ONE pass yields both units' parameter gradients; the stem's
        # output gradient (its only consumer is the stem's weight gradient) is never written (csrc/stemdw.hip)
        if (k == 3 and not self.bf16 and not self.frozen and self._sole_producer(i, xv, ("stem",), need_single=True) and self._single(nd)
                and _lib.query("mny_stemdw_supported", N, self.H, self.W, i.C, i.act, o.act) == 1):
            pu = self.units[i.id]
            sparts = _lib.query("mny_stemdw_bwd_parts", N, self.H, self.W, i.C)
            xws = torch.empty(max(int(_lib.query("mny_stemdw_bwd_ws_floats", N, self.H, self.W, i.C)), 4), **self._f32)
            _, dwv, _, _ = self._red_jobs.pop()            # the job registered above counts the rows of mny_dw_bnbwd's partial buffer
            ws_k = self._defer_job(sparts * C * 9, dwv, sparts, C * 9)
            self.bwd.add("mny_stemdw_bwd", G, u.Y, u.scale, u.shift, o.act, self.coef_ws, pu.Y, pu.scale, pu.shift, pu.mean, pu.invstd,
                         P[prod.bn + ".weight"], i.act, self.x_ptr, P[prod.conv + ".weight"], wt,
                         gv(prod.conv + ".weight"), gv(prod.bn + ".weight"), gv(prod.bn + ".bias"), None, ws_k, xws,
                         N, self.H, self.W, i.C, self.stream,
                         meta=dict(flops=2 * M * C * (2 * 9 + 27), bytes=4 * (3 * M * C + N * 3 * self.H * self.W), shape="stem+dw C%d H%d" % (C, ish[1])))
            self.stemdw_done.add(i.id)
            return
        head = (G, u.Y, u.scale, u.shift, o.act, self.coef_ws, xv[0], xv[1], xv[2], xv[3])
        geom = (N, ish[1], ish[2], C, k, 1)
        meta = dict(flops=4 * M * C * kk, bytes=self.eb * 4 * M * C, shape="C%d H%d%s" % (C, ish[1], " k5" if k == 5 else ""))
        if not with_red:
            self._contribute_kernel(i, lambda out, addend: self.bwd.add(
                self.K("mny_dw_bnbwd"), *head, wt, addend, out, dwv_k, ws_k, *geom, self.stream, meta=meta))
            return
        pu = self.units[i.id]
        rbuf = self._new_fused_red(i, _lib.query("mny_dw_bnbwd_parts_k", N, ish[1], ish[2], C, k, pflags))
        # the producer is a wide expand unit on the low-rank BN backward: it takes its gradient as ca o dX o act'(z) (mny_dw_bnbwd_red_dz)
        lr = prod.op == "pw" and self._lr_ok(prod) and _lib.query("mny_dw_bnbwd_red_dz_supported", k, C, int(self.bf16)) == 1
        if lr:
            self.lr_units.add(i.id)
        meta["shape"] += " +red" + (" dz" if lr else "")
        self._contribute_kernel(i, lambda out, addend: self.bwd.add(
            "mny_dw_bnbwd_red_dz" if lr else self.K("mny_dw_bnbwd_red"), *head, pu.mean, pu.invstd, wt, addend, out, dwv_k, ws_k, rbuf, *geom, self.stream,
            label=self.K("mny_dw_bnbwd_red"), meta=meta))

    def _bwd_dw_s2(self, nd, G):
        """3x3 stride-2 depthwise unit: the same fusion (mny_dw_bnbwd_s2): no dY tensor, one launch instead of three."""
        N = self.N
        o, u, i = nd.out, self.units[nd.out.id], nd.ins[0]
        M, C = u.M, o.C
        ish = self._shape(i)
        xv = self._view(i)
        self._bn_sums(nd, G)
        wt = self._P[nd.conv + ".weight"]
        dwv_k, ws_k = self._wgrad_dest(nd, lambda: _lib.query("mny_dw_bnbwd_s2_parts", N, ish[1], ish[2], C), C * 9, self.ws)
        head = (G, u.Y, u.scale, u.shift, o.act, self.coef_ws, xv[0], xv[1], xv[2], xv[3])
        meta = dict(flops=4 * M * C * 9, bytes=self.eb * (2 * M * C + 2 * N * ish[1] * ish[2] * C), shape="C%d H%d s2" % (C, ish[1]))
        # behind a wide expand unit on the low-rank BN backward (round 6): the producer's sums and  ca o dX o relu6'(z)  leave with this pass
        if (not self.bf16 and self._sole_producer(i, xv, ("pw",), own_sums_ok=True) and i.act == _lib.ACT_RELU6 and self._lr_ok(i.node)
                and not self.sw_no_lr_s2):
            pu = self.units[i.id]
            rbuf = self._new_fused_red(i, _lib.query("mny_dw_bnbwd_s2_parts", N, ish[1], ish[2], C))
            self.lr_units.add(i.id)
            meta["shape"] += " +red dz"
            self._contribute_kernel(i, lambda out, addend: self.bwd.add(
                "mny_dw_bnbwd_s2_red_dz", *head, pu.mean, pu.invstd, wt, addend, out, dwv_k, ws_k, rbuf, N, ish[1], ish[2], C, self.stream,
                label=self.K("mny_dw_bnbwd_s2"), meta=meta))
        else:
            self._contribute_kernel(i, lambda out, addend: self.bwd.add(
                self.K("mny_dw_bnbwd_s2"), *head, wt, addend, out, dwv_k, ws_k, N, ish[1], ish[2], C, self.stream, meta=meta))

    def _bwd_dw_s2k5(self, nd, G):
        """5x5 stride-2 depthwise unit (MobileNetV3's two down-sampling 5x5 blocks): mny_dw_bnbwd_s2k5 — one launch instead of
        bn_bwd_apply + dw5_wgrad + dw_bwd_data_s2k5, and the producer's BN-backward sums with it where the unit is its only consumer."""
        N = self.N
        o, u, i = nd.out, self.units[nd.out.id], nd.ins[0]
        M, C = u.M, o.C
        ish = self._shape(i)
        xv = self._view(i)
        self._bn_sums(nd, G)
        wt = self._P[nd.conv + ".weight"]
        dparts = _lib.query("mny_dw_bnbwd_s2k5_parts", N, ish[1], ish[2], C)
        dwv_k, ws_k = self._wgrad_dest(nd, dparts, C * 25, self.ws)
        pmean, pinvstd, rbuf = None, None, None
        if self._sole_producer(i, xv, ("pw", "stem"), no_acts=(_lib.ACT_HSIGMOID,)):
            pmean, pinvstd = self.units[i.id].mean, self.units[i.id].invstd
            rbuf = self._new_fused_red(i, dparts)
        self._contribute_kernel(i, lambda out, addend: self.bwd.add(
            self.K("mny_dw_bnbwd_s2k5"), G, u.Y, u.scale, u.shift, o.act, self.coef_ws, xv[0], xv[1], xv[2], xv[3], pmean, pinvstd, wt, addend, out, dwv_k, ws_k, rbuf,
            N, ish[1], ish[2], C, self.stream,
            meta=dict(flops=4 * M * C * 25, bytes=self.eb * (2 * M * C + 2 * N * ish[1] * ish[2] * C), shape="C%d H%d s2 k5%s" % (C, ish[1], " +red" if rbuf is not None else ""))))

    def _project_ok(self, nd):
        """linear project unit behind a conv+BN+act unit it alone consumes (the thin bottleneck that closes an inverted-residual block)."""
        o = nd.out
        if not (nd.op == "pw" and not self.frozen and o.act == ACT_NONE and not nd.bias and self._single(nd) and o.id not in self.head_cp):
            return False
        i = nd.ins[0]
        return (self._sole_producer(i, self._view(i), ("dw", "pw"), need_single=True)
                and _lib.query(self.K("mny_pj_bwd_supported"), self.units[o.id].M, i.C, o.C, i.act) == 1)

    def _bwd_project(self, nd, G):
        """Project unit (_project_ok): ONE pass rebuilds dY in LDS, reads the wide input once and yields the data gradient, the input unit's
        BN-backward sums and the weight gradient (csrc/pjbwd.hip; bf16 storage: mny_pj_bwd_bf16, csrc/gate.hip) — instead of bn_bwd_apply +
        pw_dgrad_bnred + pw_wgrad.  (G is only read here: a gradient buffer shared with the residual path is fine.)"""
        o, u, i = nd.out, self.units[nd.out.id], nd.ins[0]
        M, Ki, No = u.M, i.C, o.C
        self._bn_sums(nd, G)
        pu = self.units[i.id]
        rparts = _lib.query(self.K("mny_pj_bwd_parts"), M, Ki, No)
        rbuf = self._new_fused_red(i, rparts)
        dwv_k, ws_k = self._wgrad_dest(nd, rparts, No * Ki, None)
        self._contribute_kernel(i, lambda out, addend: self.bwd.add(
            self.K("mny_pj_bwd"), G, u.Y, self.coef_ws, pu.Y, pu.scale, pu.shift, pu.mean, pu.invstd, i.act, self._P[nd.conv + ".weight"], out, dwv_k, ws_k, rbuf,
            M, Ki, No, self.stream,
            meta=dict(flops=4 * M * Ki * No, bytes=self.eb * (2 * M * No + 2 * M * Ki), shape="project M%d K%d N%d" % (M, Ki, No))))

    def _bwd_generic(self, nd, G):
        """Any other unit, and the heads: BN sums and bn_bwd_apply -> dY (a head's G is its dY), then the weight and data gradients."""
        bwd, o = self.bwd, nd.out
        if nd.op == "pwb":
            return self._bwd_pw_grads(nd, G)
        u = self.units[o.id]
        dY = G if not self._gs[o.id].shared else self._alloc_grad(o)
        self._bn_sums(nd, G)
        if nd.op == "stem" and _lib.query("mny_stem_bnwgrad_supported", o.C) == 1:
            # the stem has no data gradient: its only consumer of dY is the weight gradient, which rebuilds dY from (G, Y) on load
            sdw, sws = self._wgrad_dest(nd, lambda: _lib.query("mny_stem_wgrad_parts", self.N, self.H, self.W, o.C), o.C * 27, self.ws)
            bwd.add(self.K("mny_stem_bnwgrad"), self.x_ptr, G, u.Y, u.scale, u.shift, o.act, self.coef_ws, sdw, sws,
                    self.N, self.H, self.W, o.C, self.stream)
            return
        bwd.add(self.K("mny_bn_bwd_apply"), G, u.Y, u.scale, u.shift, o.act, self.coef_ws, dY, u.M, o.C, self.stream,
                meta=dict(flops=0, bytes=3 * self.eb * u.M * o.C, shape="M%d C%d" % (u.M, o.C)))
        if nd.op == "stem":
            if self.side_on:
                bwd.add_py(self._fork_side, "fork")
            bwd.add(self.K("mny_stem_wgrad"), self.x_ptr, dY, self._gv(nd.conv + ".weight"), self.ws_side, self.N, self.H, self.W, o.C, self.stream_side)
        elif nd.op == "dw":
            self._bwd_dw_grads(nd, dY)
        else:
            self._bwd_pw_grads(nd, dY)

    def _bwd_dw_grads(self, nd, dY):
        """Weight and data gradient of a depthwise conv from its materialised dY."""
        bwd, N, o, i = self.bwd, self.N, nd.out, nd.ins[0]
        C, k, s = o.C, nd.k, nd.stride
        M = self._rows(o)
        ish = self._shape(i)
        xv = self._view(i)
        w = self._P[nd.conv + ".weight"]
        meta = dict(flops=2 * M * C * k * k, bytes=self.eb * (N * ish[1] * ish[2] * C + M * C), shape="C%d H%d s%d" % (C, ish[1], s))
        on_side = self.side_on and self._single(nd)          # (both contributions of a module applied twice stay in order on the main stream)
        dwv_, dws_ = self._wgrad_dest(nd, lambda: _lib.query("mny_dw_wgrad_parts", N, ish[1], ish[2], C, k, s), C * k * k,
                                      self.ws_side if on_side else self.ws)
        if on_side:
            bwd.add_py(self._fork_side, "fork")
        bwd.add(self.K("mny_dw_bwd_weight"), xv[0], xv[1], xv[2], xv[3], dY, dwv_, dws_, N, ish[1], ish[2], C,
                k, s, self.stream_side if on_side else self.stream, meta=meta)
        if not self.frontier.needs_grad(i):
            return                               # at the frontier: nothing upstream takes a gradient
        self._contribute_kernel(i, lambda out, addend: bwd.add(
            self.K("mny_dw_bwd_data"), dY, w, addend, out, N, ish[1], ish[2], C, k, s, self.stream, meta=dict(meta)))

    def _bwd_pw_grads(self, nd, dY):
        """Weight (and bias) gradient of a pointwise conv from its dY, then the data gradient in one of three forms: with the BN-backward
        sums of the unit whose complete output gradient it is (mny_pw_dgrad_bnred), the same with earlier contributions as the addend
        (_add), or the plain GEMM."""
        bwd, K, eb = self.bwd, self.K, self.eb
        o, i = nd.out, nd.ins[0]
        oc = self.head_cp.get(o.id, o.C)        # channel count of dY as the GEMMs see it (padded for the heads)
        M = self._rows(o)
        xv = self._view(i)
        db = self._gv(nd.conv + ".bias") if nd.bias else None
        on_side = self.side_on and self._single(nd)          # (both contributions of a module applied twice stay in order on the main stream)
        dwv_, pws_ = self._wgrad_dest(nd, lambda: _lib.query(K("mny_pw_wgrad_splits"), M, i.C, oc), oc * i.C, self.ws_side if on_side else self.ws,
                                      floats=lambda p: max(_lib.query("mny_pw_wgrad_ws_floats", M, i.C, oc), p * oc * i.C), also=db is None)
        if on_side:
            bwd.add_py(self._fork_side, "fork")
        bwd.add(K("mny_pw_wgrad"), xv[0], xv[1], xv[2], xv[3], dY, dwv_, db, pws_, M, i.C, oc,
                self.stream_side if on_side else self.stream,
                meta=dict(flops=2 * M * i.C * o.C, bytes=eb * (M * i.C + M * o.C) + 4 * i.C * o.C, shape="M%d K%d N%d" % (M, i.C, oc)))
        if not self.frontier.needs_grad(i):
            return                               # at the frontier: nothing upstream takes a gradient
        wT = self.wT[nd.conv]                   # filled by the batched transpose at the head of the list
        wT6 = self.wT6.get(nd.conv)             # pre-cut W^T planes: this data gradient takes the six-product bf16 form
        # (bf16 storage: round 2 measured the epilogue's 2-byte loads of the unit's output at what the saved pass cost, 3 281 vs
        # 3 293 img/s on MobileNetV3 512; with round 3's kernels it wins — same-box A/B 17.65-17.70 vs 17.93-17.99 ms/step — and is on)
        # the unit whose complete output gradient this data gradient is (i itself, or — through a residual add — the add's unit operand)
        tgt = self._red_target(i, nd)
        # this data gradient IS the complete dL/d(output) of a conv+BN+act unit whose backward starts with a BN reduction:
        # the sums are taken from the GEMM's own output tile (+ the unit's raw output), the separate reduce pass is dropped ...
        form = None
        if tgt is not None and self._gs[i.id].buf is None and _lib.query(K("mny_pw_dgrad_bnred_supported"), M, oc, i.C, tgt.act) == 1:
            form = "mny_pw_dgrad_bnred"
        # ... or it is the LAST contribution to the output gradient of such a unit (a project conv feeding a residual add and the
        # next block — or the block input that IS that residual sum): the earlier contributions arrive as the addend, the epilogue
        # sees the complete gradient -> BN sums here
        elif tgt is not None and self._gs[i.id].buf is not None and _lib.query(K("mny_pw_dgrad_bnred_add_supported"), M, oc, i.C, tgt.act) == 1:
            form = "mny_pw_dgrad_bnred_add"
        if form is None:
            self._contribute_kernel(i, lambda out, addend: self._emit_pw_gemm(
                bwd, (dY, None, None, ACT_NONE), wT6 if wT6 is not None else wT, wT6 is not None, None, addend, out, None, M, oc, i.C, self.stream, tag="dgrad "))
            return
        add = form.endswith("_add")
        pu = self.units[tgt.id]
        assert tgt.C == i.C
        rbuf = self._new_fused_red(tgt, _lib.query(K("mny_pw_dgrad_bnred_parts"), M, oc, i.C))
        tail = (pu.Y, pu.scale, pu.shift, tgt.act, pu.mean, pu.invstd, rbuf, M, oc, i.C, self.stream)
        meta = dict(flops=2 * M * oc * i.C, bytes=eb * (M * oc + (3 if add else 2) * M * i.C) + 4 * oc * i.C,
                    shape="dgrad+%sred M%d K%d N%d" % ("add+" if add else "", M, oc, i.C))

        def emit(out, addend):
            if wT6 is not None:                 # the _w6 entry point takes the addend in both forms (NULL without one)
                bwd.add("mny_pw_dgrad_bnred_w6", dY, wT6, addend if add else None, out, *tail, label=form, meta=meta)
            elif add:
                bwd.add(K(form), dY, wT, addend, out, *tail, meta=meta)
            else:
                bwd.add(K(form), dY, wT, out, *tail, meta=meta)
        self._contribute_kernel(i, emit)

    # ------------------------------------------------------------------------------------------
    def _w6_planes(self, w2d, M, K, Nc):
        """Plane buffer for the weight operand `w2d` ([Nc][K] fp32) of a GEMM that takes the six-product bf16 form (fp32 plans), or None."""
        if self.bf16 or _lib.query("mny_pw_w6_supported", M, K, Nc) != 1:
            return None
        planes = torch.empty(_lib.query("mny_pw_w6_bytes", K, Nc), device=self.dev, dtype=torch.uint8)
        self._cut_jobs.append((w2d, planes, Nc, K))
        return planes

    def _job_table(self, rows, fields, block_job=None):
        """Device copies of the packed job table of a batched launch (`rows` as the C struct `fields`, as bytes) and of its
        block -> job map (int32; None without one)."""
        jt = np.array(rows, dtype=np.dtype(fields))
        jdev = torch.from_numpy(jt.view(np.uint8).copy()).to(self.dev)
        return jdev, (torch.tensor(block_job, dtype=torch.int32, device=self.dev) if block_job is not None else None)

    def _flush_cut_jobs(self, calls, at_head=False):
        """One mny_cut3_batch launch for the pending (matrix, planes) pairs; at_head: placed first in the list (forward weights)."""
        if not self._cut_jobs:
            return
        rows, block_job = [], []
        for src, planes, R, C in self._cut_jobs:
            rows.append((src.data_ptr(), planes.data_ptr(), R, C, len(block_job), 0))
            block_job += [len(rows) - 1] * ((R * ((C + 15) // 16) * 2 + 255) // 256)
        jd, bj = self._job_table(rows, [("src", np.uint64), ("dst", np.uint64), ("R", np.int32), ("C", np.int32), ("b0", np.int32), ("pad", np.int32)], block_job)
        calls.add("mny_cut3_batch", jd, bj, len(block_job), self.stream)
        if at_head:
            calls.calls.insert(0, calls.calls.pop())
        calls.keep += [t for job in self._cut_jobs for t in job[:2]]
        self._cut_jobs = []

    def _gemm_weight(self, w):
        """Weight operand of a forward pointwise GEMM: the fp32 parameter itself, or (bf16 storage) a bf16 shadow copy
        refreshed by a conversion call placed right before the GEMM — the fp32 master copy is what optimizers update."""
        if not self.bf16:
            return w
        w16 = torch.empty(w.shape, device=self.dev, dtype=torch.bfloat16)
        self._cvt_jobs.append((w, w16))              # one batched conversion at the head of the forward list (_flush_cvt_jobs)
        return w16

    def _flush_cvt_jobs(self):
        if not self._cvt_jobs:
            return
        rows, block_job = [], []
        for w, w16 in self._cvt_jobs:
            rows.append((w.data_ptr(), w16.data_ptr(), w.numel(), len(block_job), 0))
            block_job += [len(rows) - 1] * ((w.numel() + 4095) // 4096)
        self.c_jobs, self.c_blocks = self._job_table(rows, [("src", np.uint64), ("dst", np.uint64), ("n", np.int64), ("b0", np.int32), ("pad", np.int32)], block_job)
        self.fwd.add("mny_cvt_batch_f32_bf16", self.c_jobs, self.c_blocks, len(block_job), self.stream)
        self.fwd.calls.insert(0, self.fwd.calls.pop())       # the shadows must exist before the first GEMM
        self.fwd.keep += [t for pair in self._cvt_jobs for t in pair]

    def K(self, name):
        """Entry point for the plan's activation storage type."""
        return name + "_bf16" if self.bf16 else name

    def kernel_routes(self):
        """[(entry point as called, label, (M, K, N), mny_pw_route family)] for every pointwise-conv call of the plan's two lists —
        which kernel family each launch takes (tests assert that a plan compared with the oracle contains the families the benchmark
        runs; tools/plan_stats.py prints the table)."""
        out = []
        lists = [("fwd", self.fwd.calls)] + ([("bwd", self.bwd.calls)] if self.bwd is not None else [])
        for which, calls in lists:
            for idx, (fn, _args, label, meta) in enumerate(calls):
                base = label[:-5] if label.endswith("_bf16") else label
                op = {"mny_pw_fwd": 0, "mny_pw_dgrad_bnred": 1, "mny_pw_dgrad_bnred_add": 1, "mny_pw_wgrad": 2}.get(base)
                m = re.search(r"M(\d+) K(\d+) N(\d+)", (meta or {}).get("shape", ""))
                if op is None or m is None:
                    continue
                M, K, N = (int(v) for v in m.groups())
                fam = self.routes[which].get(idx)             # what the dispatcher did; the predictor only before the first replay
                if fam is None:
                    fam = _lib.query("mny_pw_route", op, int(self.bf16), M, K, N)
                out.append((getattr(fn, "__name__", label), label, (M, K, N), fam))
        return out

    def stale(self):
        return any(t.data_ptr() != p for t, p in self.param_ptrs)

    def _bind(self, x):
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and tuple(x.shape) == (self.N, 3, self.H, self.W)
        if self.use_graphs:                      # graphs bake pointers: stage the batch in a resident buffer (0.15 ms at bs=256)
            if self.x_static is None:
                self.x_static = torch.empty_like(x)
            if x.data_ptr() != self.x_static.data_ptr():
                self.x_static.copy_(x)
            x = self.x_static
        self.x_ptr.value = x.data_ptr()
        self.stream.value = torch.cuda.current_stream(self.dev).cuda_stream
        return x

    def _replay(self, which, calls, begin=0, end=None):
        """Run calls[begin:end]: HIP-event bracketed (bench), as a captured hipGraph, or eagerly."""
        if self.timing is not None:
            calls.run_timed(self.timing[which], self.timing["only"], begin, end)
            return
        if not (self.use_graphs and self.eager_steps >= 2):
            key = (which, begin, end)
            if key not in self._recorded:
                calls.run_recording(self.routes[which], begin, end)          # the first replay of every segment: which kernel family each dispatcher took
                self._recorded.add(key)
            else:
                calls.run(begin, end)
            return
        key = (which, begin, end)
        g = self.graphs.get(key)
        if g is None:
            cur = torch.cuda.current_stream(self.dev)
            try:
                g = torch.cuda.CUDAGraph()
                side = torch.cuda.Stream(self.dev)
                with torch.cuda.graph(g, stream=side):
                    self.stream.value = torch.cuda.current_stream(self.dev).cuda_stream
                    calls.run(begin, end)
            except Exception as e:               # noqa: BLE001 — capture is an optimisation, never a requirement
                warnings.warn("hipGraph capture failed (%s); staying on the eager call list" % (e,))
                self.use_graphs = False
                self.graphs.clear()
                self.stream.value = cur.cuda_stream
                calls.run(begin, end)
                return
            finally:
                self.stream.value = cur.cuda_stream
            self.graphs[key] = g
        g.replay()

    def set_targets(self, targets):
        """targets: list (len N) of [n_i,5] float tensors (label,cx,cy,w,h), CPU or device."""
        assert len(targets) == self.N, "need one target tensor per image"
        counts = [int(t.shape[0]) for t in targets]
        total = sum(counts)
        if total > self.t_dev.shape[0]:
            self.t_dev = torch.zeros(2 * total, 5, device=self.dev, dtype=torch.float32)
            self.graphs.clear()                  # captured graphs hold the old buffer's address
        acc, offs = 0, [0]
        for c in counts:
            acc += c
            offs.append(acc)
        off = torch.tensor(offs, dtype=torch.int32)
        if total:
            packed = torch.cat([t.reshape(-1, 5) for t in targets if t.shape[0]]).to(torch.float32)
            self.t_dev[:total].copy_(packed, non_blocking=True)
        self.off_dev.copy_(off, non_blocking=True)
        self.t_ptr.value = self.t_dev.data_ptr()
        self.off_ptr.value = self.off_dev.data_ptr()

    def forward_train(self, x, targets, seg_maps=None):
        x = self._bind(x)
        self.stream_side.value = self._side_stream.cuda_stream if (self.side_on and self.timing is None) else self.stream.value
        self.stream_side2.value = self._side2_stream.cuda_stream if (self.side_on and self.timing is None) else self.stream.value
        self.set_targets(targets)
        if self.seg_head is not None:
            if seg_maps is None:
                raise ValueError("this config has a `seg` section: training needs seg_maps [N,h,w,C] (train.py:257-258)")
            if tuple(seg_maps.shape) != tuple(self.seg_maps.shape):
                raise ValueError("seg_maps must be %s (N, H/16, W/16, seg classes), got %s" % (tuple(self.seg_maps.shape), tuple(seg_maps.shape)))
            self.seg_maps.copy_(seg_maps, non_blocking=True)                    # seg_loss.py:53 (clone().to(device))
        self._replay("fwd", self.fwd)
        self.saved_x = x
        self.fwd_gen += 1
        self.last_fwd_tick = next(_FWD_TICK)
        return self.out14

    def backward(self, g_losses):
        self.stream.value = torch.cuda.current_stream(self.dev).cuda_stream
        # event-bracketed runs (bench breakdown) keep everything on one stream so the brackets mean something
        self.stream_side.value = self._side_stream.cuda_stream if (self.side_on and self.timing is None) else self.stream.value
        self.stream_side2.value = self._side2_stream.cuda_stream if (self.side_on and self.timing is None) else self.stream.value
        self.x_ptr.value = self.saved_x.data_ptr()
        self.g_scale.copy_(g_losses.reshape(self.g_scale.numel()).to(self.g_scale.dtype))
        if self.reducer is not None:
            self.reducer.run_backward()             # segmented replay + bucketed RCCL all-reduce (dp.py)
        else:
            self.run_bwd_segment(0, None)
        self.eager_steps += 1

    def _fork_side(self):
        # one fork and one join event per plan, reused by every fork / join of a step (a wait captures the record that precedes it, so
        # re-recording the same event later is safe): round 2 created ~70 fresh torch.cuda.Event objects per step
        if self.side_on and self.timing is None:
            self._ev_fork.record(torch.cuda.current_stream(self.dev))
            self._side_stream.wait_event(self._ev_fork)
            self._side_used = True

    def _fork_side2(self):
        if self.side_on and self.timing is None:
            self._ev_fork2.record(torch.cuda.current_stream(self.dev))
            self._side2_stream.wait_event(self._ev_fork2)

    def _join_side2(self):
        if self.side_on and self.timing is None:
            self._ev_join2.record(self._side2_stream)
            torch.cuda.current_stream(self.dev).wait_event(self._ev_join2)

    def _join_side(self):
        if self._side_used:
            self._ev_join.record(self._side_stream)
            torch.cuda.current_stream(self.dev).wait_event(self._ev_join)
            self._side_used = False

    def run_bwd_segment(self, begin, end):
        self._replay("bwd", self.bwd, begin, end)
        self._join_side()                                    # gradients of this segment are complete on the main stream

    def enable_timing(self, only=None, steps=1):
        """Bracket calls with HIP events (bench.py roofline leg); disable with disable_timing().  `steps`: how many steps will
        be recorded before the events are read — their events are created here, outside the timed region."""
        sel = set(only) if only else None
        n = sum(1 for cl in (self.fwd, self.bwd) for c in cl.calls if sel is None or c[2] in sel)
        HipEvent.reserve(2 * n * max(int(steps), 1))
        self.timing = {"fwd": [], "bwd": [], "only": sel}

    def disable_timing(self):
        t, self.timing = self.timing, None
        return t

    def forward_eval(self, x, val_conf, nms=True, decode=True):
        """`nms=False` leaves the plan's own NMS out (the caller runs one over several plans' candidates, tta.py): rows / cnt1 hold the
        decoded candidates, out_idx / out_counts / out_rows are not written.  `decode=False` leaves the plan's decode out as well (the
        caller decodes `heads` itself, postprocess.py): only the forward and the seg head's sigmoid run, rows / cnt0 / cnt1 are untouched."""
        x = self._bind(x)
        self.fwd.run()
        for i in range(2):
            self.val_conf[i].value = val_conf[i]
        if not decode:
            self.det.run(self.det_nms + 1)
        elif nms:
            self.det.run()
        else:
            self.det.run(0, self.det_nms)
            self.det.run(self.det_nms + 1)
