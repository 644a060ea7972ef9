#!/usr/bin/env python3
"""Times the fused SGD step, the EMA update and the EMA swap pair on the model's real parameter set against torch's foreach forms.

    python examples/time_optim.py [--arch mbv2|mbv3] [--reps 50] [--warmup 10] [--rounds 5] [--chunks 65536,32768,16384,8192,4096]

One backward at bs 4, 160x160 gives every trainable parameter its arena-view gradient.  Each figure is the HIP-event time of `reps`
back-to-back calls divided by `reps`, after `warmup` calls — the cost of the call in a training loop, host enqueue included (torch's
foreach forms are several launches per call) — and the median of `rounds` such windows, the variants taking turns.  The fused forms are
timed once per chunk length of `--chunks`; the headline figures are those of optim.STREAM_CHUNK.  The `*_kernel_us` figures are the
three entry points called back to back on the cached tables (no Python walk over the tensors between launches): the device side alone,
which is where the chunk length shows.  Prints one JSON line.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mobilenet_yolo_pytorch_amd import _lib, mbv3, optim, synthetic, yolo  # noqa: E402


def window(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps          # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="mbv2", choices=["mbv2", "mbv3"])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--chunks", default="65536,32768,16384,8192,4096")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_optim.py needs the MI355X"
    torch.manual_seed(0)
    model = (yolo if a.arch == "mbv2" else mbv3.yolo)(synthetic.VOC_CONFIG).cuda().train()
    out = model(synthetic.images(4, 160, 160, seed=1).cuda(), synthetic.targets(4, seed=2, empty_every=0))
    sum(o[0] for o in out).backward()
    kw = dict(lr=1e-6, momentum=0.9, nesterov=True, weight_decay=5e-4)

    ref = [torch.nn.Parameter(p.detach().clone()) for p in model.parameters()]
    for r, p in zip(ref, model.parameters()):
        r.grad = None if p.grad is None else p.grad.detach().clone()
    stock = torch.optim.SGD(ref, foreach=True, **kw)
    live = [v.detach() for v in model.state_dict(keep_vars=True).values() if v.is_floating_point()]
    shadow = [t.clone() for t in live]
    variants = {"sgd_torch_foreach_us": stock.step, "ema_foreach_lerp_us": lambda: torch._foreach_lerp_(shadow, live, 1e-4)}

    chunks = [int(c) for c in a.chunks.split(",")]
    if optim.STREAM_CHUNK not in chunks:
        chunks.append(optim.STREAM_CHUNK)
    default = optim.STREAM_CHUNK
    for c in chunks:                                 # a fused optimizer / EMA per chunk length: tables are built with the length in force
        optim.STREAM_CHUNK = c
        fused, ema = optim.SGD(model.parameters(), **kw), optim.ModelEMA(model)
        fused.step(); fused.step(); ema.update()     # past the first-step table; tables built

        def swap_pair(ema=ema):
            with ema.applied():
                pass
        variants["sgd_fused_us@%d" % c] = fused.step
        variants["ema_fused_us@%d" % c] = ema.update
        variants["swap_pair_us@%d" % c] = swap_pair
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        (sub,), (etab, en, _dev) = fused._tables[0][1], ema._table()
        stab, sn, eptr = ctypes.c_void_p(sub["table"].data_ptr()), sub["nchunks"], ctypes.c_void_p(etab.data_ptr())
        variants["sgd_kernel_us@%d" % c] = lambda stab=stab, sn=sn: _lib.call("mny_sgd_step", stab, sn, 1e-6, 0.9, 0.0, 5e-4, 1, 0, st)
        variants["ema_kernel_us@%d" % c] = lambda eptr=eptr, en=en: _lib.call("mny_ema_update", eptr, en, 0.9998, st)
        variants["swap_kernel_us@%d" % c] = lambda eptr=eptr, en=en: _lib.call("mny_swap_chunks", eptr, en, st)
    optim.STREAM_CHUNK = default

    times = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            times[k].append(window(fn, a.reps, a.warmup))
    med = {k: round(statistics.median(v), 2) for k, v in times.items()}
    spread = {k: round(max(v) - min(v), 2) for k, v in times.items()}
    res = {"arch": a.arch, "tensors_with_grad": sum(p.grad is not None for p in model.parameters()), "ema_tensors": len(live),
           "parameters": sum(p.numel() for p in model.parameters()), "reps": a.reps, "warmup": a.warmup, "rounds": a.rounds, "chunk": default}
    for k in ("sgd_fused_us", "ema_fused_us", "swap_pair_us", "sgd_kernel_us", "ema_kernel_us", "swap_kernel_us"):
        res[k] = med["%s@%d" % (k, default)]
        res[k[:-3] + "_by_chunk_us"] = {str(c): med["%s@%d" % (k, c)] for c in chunks}
    res["sgd_torch_foreach_us"], res["ema_foreach_lerp_us"] = med["sgd_torch_foreach_us"], med["ema_foreach_lerp_us"]
    res["max_spread_us"] = max(spread.values())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
