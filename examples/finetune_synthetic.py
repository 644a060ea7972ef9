#!/usr/bin/env python3
"""Fine-tuning with a frozen backbone on synthetic data: what a step costs when only the neck and the heads train.

    python examples/finetune_synthetic.py [--batch 256] [--size 352] [--steps 20] [--warmup 5] [--clip 10.0]

Runs the full training step and the frozen-backbone step (requires_grad_(False) on the backbone and backbone.eval(), so its BatchNorm
layers keep their statistics) on the same fp32 batch, with the discipline of bench.py: warm-up steps, then timed steps
(zero_grad -> forward + losses -> backward) between two device synchronisations.  Prints ms/step and the number of backward calls
of both, then clips the frozen step's gradients with optim.clip_grad_norm_.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mobilenet_yolo_pytorch_amd import optim, synthetic, yolo  # noqa: E402


def timed_steps(model, x, tg, warmup, steps):
    def step():
        model.zero_grad(set_to_none=True)
        out = model(x, tg)
        (out[0][0] + out[1][0]).backward()
        return out
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    plan = next(p for p in reversed(list(model._plans.values())) if p.bwd is not None)
    n_bwd = sum(1 for c in plan.bwd.calls if c[2] not in ("fork", "join"))          # library calls (the rest are stream forks / joins)
    return ms, n_bwd, len(plan.grad_params), float((out[0][0] + out[1][0]).detach())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=352)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--clip", type=float, default=10.0)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = yolo(synthetic.VOC_CONFIG).to(dev).train()
    x = synthetic.images(a.batch, a.size, a.size, seed=0).to(dev)
    tg = synthetic.targets(a.batch, seed=1, empty_every=16)
    full = timed_steps(model, x, tg, a.warmup, a.steps)
    print("full step            : %7.2f ms/step  %4d backward calls  %3d gradient tensors  loss %.5f" % full)
    model._plans.clear()                                   # one resident plan at a time at this batch size
    for p in model.backbone.parameters():
        p.requires_grad_(False)
    model.backbone.eval()                                  # keep the backbone's BatchNorm statistics
    frozen = timed_steps(model, x, tg, a.warmup, a.steps)
    print("frozen-backbone step : %7.2f ms/step  %4d backward calls  %3d gradient tensors  loss %.5f" % frozen)
    print("frozen / full        : %.3f" % (frozen[0] / full[0]))
    assert all(p.grad is None for p in model.backbone.parameters())
    norm = optim.clip_grad_norm_(model, a.clip)
    print("clip_grad_norm_(model, %g): total norm %.5f" % (a.clip, float(norm)))


if __name__ == "__main__":
    main()
