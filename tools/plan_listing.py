"""Canonical text listing of a plan's call lists, for comparing two checkouts byte for byte.

usage:  python tools/plan_listing.py CHECKOUT CASE [CASE ...] [--device cpu|cuda]
  CHECKOUT  root of the checkout whose package builds the plans (one copy of this tool lists any commit, e.g. from a `git worktree`)
  CASE      arch:dtype:N:size[:mode]   arch = mbv2 | mbv3 | bdd (MobileNetV2 with the BDD100K config of tests/golden)
                                       dtype = f32 | bf16      mode = train (default) | frozen | eval

One line per call: list, index, entry point actually called, label, every argument, the meta dict; then bwd.marks, grad_params and
grad_slots.  A tensor is written as dtype, shape and the ordinal at which its address was first seen in the listing
(inside the gradient arena: g + its float offset), ints and floats by
value, host callables by name.  The listing does not show the contents of device job tables.

engine.CallList is replaced by a recording subclass whose add() keeps the arguments as given and does not insist on device tensors, so
plans also build on CPU tensors (MNY_SIDE_STREAM=0: a side stream is a device object).  Nothing else of the package is touched.
"""
import ctypes
import hashlib
import json
import os
import sys

import torch


def recording_call_list(engine):
    """engine.CallList with add() recording its arguments as given (raw[id(call tuple)]) and accepting CPU tensors."""
    class RecordingCallList(engine.CallList):
        def __init__(self):
            super().__init__()
            self.raw = {}

        def add(self, name, *args, meta=None, label=None):
            fn = getattr(engine._lib.load(), name)
            conv = []
            for a in args:
                if isinstance(a, torch.Tensor):
                    assert a.is_contiguous(), name
                    self.keep.append(a)
                    conv.append(ctypes.c_void_p(a.data_ptr()))
                else:
                    conv.append(a)
            entry = (fn, tuple(conv), label or name, meta)
            self.calls.append(entry)
            self.raw[id(entry)] = args
    return RecordingCallList


def load_engine(checkout):
    """The engine module of `checkout`, with the recording call list in place."""
    checkout = os.path.abspath(checkout)
    if checkout not in sys.path:
        sys.path.insert(0, checkout)
    import mobilenet_yolo_pytorch_amd.engine as engine
    assert os.path.abspath(engine.__file__).startswith(checkout + os.sep), engine.__file__
    if engine.CallList.__name__ != "RecordingCallList":
        engine.CallList = recording_call_list(engine)
    return engine


def build_plan(checkout, arch, dtype, N, size, mode="train", device="cpu"):
    engine = load_engine(checkout)
    from mobilenet_yolo_pytorch_amd import mbv3, synthetic, yolo
    cfg = synthetic.VOC_CONFIG
    if arch == "bdd":
        with open(os.path.join(checkout, "tests", "golden", "state_keys_bdd100k.json")) as f:
            cfg = json.load(f)["config"]
    dt = {"f32": torch.float32, "bf16": torch.bfloat16}[dtype]
    torch.manual_seed(0)
    model = (mbv3.yolo if arch == "mbv3" else yolo)(cfg, act_dtype=dt).to(device).train()
    kw = {"train": {}, "frozen": dict(bn_batch=False, frozen_bwd=True), "eval": {}}[mode]
    return engine.NetPlan(model, N, size, size, mode != "eval", dt, **kw)


class _Namer:
    """Addresses and host objects -> ordinals in order of first appearance."""

    def __init__(self, plan):
        self.addr, self.objs = {}, {}
        self.named = {id(getattr(plan, n)): n for n in ("stream", "stream_side", "stream_side2", "x_ptr", "t_ptr", "off_ptr") if hasattr(plan, n)}

        gflat = getattr(plan, "gflat", None)                   # addresses inside the gradient arena are written as their float offset
        self.g0 = gflat.data_ptr() if gflat is not None else 0
        self.g1 = self.g0 + 4 * gflat.numel() if gflat is not None else 0

    def address(self, p):
        if self.g0 <= p < self.g1:
            return "g%d" % ((p - self.g0) // 4)
        return "%d" % self.addr.setdefault(p, len(self.addr))

    def arg(self, a):
        if isinstance(a, torch.Tensor):
            return "%s%s@%s" % (str(a.dtype).replace("torch.", ""), list(a.shape), self.address(a.data_ptr()))
        if a is None or isinstance(a, (bool, int, str)):
            return repr(a)
        if isinstance(a, float):
            return repr(a)
        if isinstance(a, (ctypes.c_float, ctypes.c_double)):
            return "%s(%r)" % (type(a).__name__, a.value)
        if id(a) in self.named:
            return "ptr:" + self.named[id(a)]
        inner = getattr(a, "_obj", None)                       # ctypes.byref(struct)
        if isinstance(inner, ctypes.Structure):
            return "byref(%s)" % ",".join("%s=%r" % (f[0], getattr(inner, f[0])) for f in inner._fields_)
        if callable(a):
            return getattr(a, "__name__", type(a).__name__)
        return "%s#%d" % (type(a).__name__, self.objs.setdefault(id(a), len(self.objs)))

    def meta(self, m):
        if m is None:
            return "-"
        out = []
        for k in sorted(m):
            v = m[k]
            if k == "writes":                                  # raw addresses of the combine's destinations
                v = "[" + ", ".join(self.address(p) for p in v) + "]"
            out.append("%s=%s" % (k, v if k == "writes" else repr(v)))
        return "{" + ", ".join(out) + "}"


def listing(plan):
    """The canonical lines of a plan built on recording call lists."""
    nm = _Namer(plan)
    lines = []
    for which in ("fwd", "bwd", "det"):
        cl = getattr(plan, which, None)
        if cl is None:
            continue
        for idx, entry in enumerate(cl.calls):
            fn, args, label, meta = entry
            raw = cl.raw.get(id(entry))
            if raw is None:                                    # add_py: a host step
                lines.append("%s %d py:%s %s" % (which, idx, getattr(fn, "__name__", "?"), label))
                continue
            lines.append("%s %d %s %s (%s) %s" % (which, idx, getattr(fn, "__name__", label), label, ", ".join(nm.arg(a) for a in raw), nm.meta(meta)))
    if getattr(plan, "bwd", None) is not None:
        lines.append("marks " + " ".join("%s=%d" % kv for kv in plan.bwd.marks.items()))
        lines.append("grad_params " + " ".join(plan.grad_params))
        lines.append("grad_slots " + " ".join("%s=%d+%d" % (n, o, c) for n, (o, c) in plan.grad_slots.items()))
        lines.append("gflat %d" % plan.gflat.numel())
    return lines


def main(argv):
    device = "cpu"
    if "--device" in argv:
        k = argv.index("--device")
        device = argv[k + 1]
        del argv[k:k + 2]
    checkout, cases = argv[0], argv[1:]
    for case in cases:
        f = case.split(":")
        arch, dtype, N, size = f[0], f[1], int(f[2]), int(f[3])
        mode = f[4] if len(f) > 4 else "train"
        plan = build_plan(checkout, arch, dtype, N, size, mode, device)
        lines = listing(plan)
        print("# case %s: %d lines, sha1 %s" % (case, len(lines), hashlib.sha1("\n".join(lines).encode()).hexdigest()))
        print("\n".join(lines))
        del plan


if __name__ == "__main__":
    main(sys.argv[1:])
