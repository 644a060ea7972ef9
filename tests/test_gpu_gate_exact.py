"""The densest kernels of the MobileNetV3 bf16 path — gate_fwd_kernel and gate_bwd_kernel, passes 1-3 at the three gate shapes, and the five
instantiations of pj16_bwd_kernel (csrc/gate.hip) — held to EQUALITY with an fp64 reference, at ragged sizes and past the first trip of their loops.

They share one machinery: a wave owns 16 pixels and all channels; accumulators are reused as the next product's B fragment; weight chunks are cut into
a private k order; padding channels vanish through zero constant rows; pixels past M are redirected to row 0 and masked; the weight gradients contract
over 128 pixels that eight waves park transposed in LDS; accumulators are carried across the trips of a grid-stride loop.  tests/test_gpu_gate.py and
the bf16 half of tests/test_gpu_pjbwd.py hold them with seeded normal data to 1e-2 (2e-3) of the reference's global maximum: a wrong tile of small
entries or a masked tail lane that leaks into dW2 fits inside (tests/test_gate_regimes_cpu.py measures what that bound sees of a leaking tail and of
stale LDS columns), and the forward residual operand with an activation, a cut of several jobs, M < 16, a second trip of pj16 <16,16>, <64,24>,
<72,40> and a call without dw were never run at all.

Every BatchNorm constant of these passes is a pointer, so the inputs of tests/gate_exact_ref.py make all arithmetic exact in fp32 (asserted on the
CPU, with every partial row's sum below 2^24 units of its accumulator whatever the order) and the reference applies bf16 round-to-nearest-even where
the kernels do.  Outputs and partial rows are pre-filled with NaN, each partial buffer one row longer than the query says: exactly the counted rows are
written, the fp64 sum of the rows and every element of out / dt / gd are EQUAL to the reference.  The rows and the regime each is there for:
tests/gate_regimes.py; every test asserts its row's regime first, from the restatement and from the library's queries.
"""
import ctypes
import time

import numpy as np
import pytest
import torch

import gate_exact_ref as ge
import gate_regimes as gr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from mobilenet_yolo_pytorch_amd import _lib
    return _lib


def _ids(rows):
    return [pytest.param(r, id=r.id) for r in rows]


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _nan(*shape, bf=False):
    return torch.full(shape, float("nan"), dtype=torch.bfloat16 if bf else torch.float32, device="cuda")


def _dev(t, bf=False):
    return None if t is None else t.to(torch.bfloat16 if bf else torch.float32).cuda().contiguous()


def _host(t):
    return t.cpu().double()


def _regime(lib, r):
    gs = gr.check_regime(r)
    for name, args, want in gr.queries(r):
        assert lib.query(name, *args) == want, (r.id, name, args, want)
    return gs


def _rows_written(buf, gx, what):
    """buf [gx + 1, ...] pre-filled with NaN: the gx counted rows are written, the extra one is not; returns the fp64 sum of the rows"""
    h = _host(buf)
    assert not torch.isnan(h[:gx]).any(), what + ": a counted partial row was not written"
    assert torch.isnan(h[gx]).all(), what + ": a row past the counted ones was written"
    return h[:gx].sum(0)


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = ~(got == want)                                  # (a NaN left in `got` is unequal too)
    if bad.any():
        idx = bad.nonzero()
        raise AssertionError("%s: %d of %d elements differ; first at %s: got %r, want %r" % (
            what, idx.shape[0], got.numel(), idx[0].tolist(), got[tuple(idx[0])].item(), want[tuple(idx[0])].item()))


def _cut(lib, jobs):
    """mny_gate_cut_batch_bf16 over [(w1 [R, C], w2 [C, R])] device tensors in ONE launch -> the chunk buffers (pre-filled with 0xff bytes)"""
    wqs = [torch.full((int(lib.query("mny_gate_wq_bytes", w1.shape[1], w1.shape[0])),), 255, device="cuda", dtype=torch.uint8) for (w1, w2) in jobs]
    rec = np.array([(w1.data_ptr(), w2.data_ptr(), wq.data_ptr(), w1.shape[1], w1.shape[0]) for (w1, w2), wq in zip(jobs, wqs)],
                   dtype=np.dtype([("w1", np.uint64), ("w2", np.uint64), ("wq", np.uint64), ("C", np.int32), ("R", np.int32)]))
    jd = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
    lib.call("mny_gate_cut_batch_bf16", _p(jd), len(jobs), _st())
    torch.cuda.synchronize()
    return wqs


@pytest.mark.parametrize("r", _ids(gr.GATE_TABLE))
def test_gate_passes_are_exact(lib, r):
    """stats1, stats2, fwd with the four residual operands (none; plain; scale and shift; scale, shift and ReLU), bwd1, bwd2, bwd3 with and without the
    project unit's BN-backward sums (red3, where mny_gate_bwd_red3_supported).  No mny_bn_finalize / mny_bn_bwd_finalize: every constant comes from
    the generator."""
    t0 = time.time()
    gs = _regime(lib, r)
    gf, gb = gs["fwd"], gs["bwd"]
    M, C, R = r.M, r.C, r.R
    assert lib.query("mny_gate_supported", M, C, R) == 1
    c = ge.gate_case(M, C, R)
    want = ge.gate_ref(c)[0]
    t1 = time.time()
    d = {k: _dev(c[k]) for k in ("s3", "b3", "w1", "w2", "sc1", "sh1", "sc2", "sh2", "mean1", "invstd1", "mean2", "invstd2", "mean3", "invstd3", "coef1", "coef2")}
    y3, dout = _dev(c["y3"], bf=True), _dev(c["dout"], bf=True)
    wq, = _cut(lib, [(d["w1"], d["w2"])])
    # forward
    st1, st2 = _nan(gf.gx + 1, 2, R), _nan(gf.gx + 1, 2, C)
    lib.call("mny_gate_stats1_bf16", _p(y3), _p(d["s3"]), _p(d["b3"]), _p(wq), _p(st1), M, C, R, _st())
    lib.call("mny_gate_stats2_bf16", _p(y3), _p(d["s3"]), _p(d["b3"]), _p(wq), _p(d["sc1"]), _p(d["sh1"]), _p(st2), M, C, R, _st())
    outs = {}
    add = dict(x=_dev(c["add_x"], bf=True), scale=_dev(c["add_scale"]), shift=_dev(c["add_shift"]))      # (alive until the synchronize below)
    for kind in ge.RESIDUALS:
        ax, asc, ash, aact = ge.residual(c, kind)
        outs[kind] = _nan(M, C, bf=True)
        lib.call("mny_gate_fwd_bf16", _p(y3), _p(d["s3"]), _p(d["b3"]), _p(wq), _p(d["sc1"]), _p(d["sh1"]), _p(d["sc2"]), _p(d["sh2"]),
                 _p(add["x"] if ax is not None else None), _p(add["scale"] if asc is not None else None), _p(add["shift"] if ash is not None else None),
                 aact, _p(outs[kind]), M, C, R, _st())
    # backward
    red2, red1 = _nan(gb.gx + 1, 2, C), _nan(gb.gx + 1, 2, R)
    dw2p, dw1p, dw1q = _nan(gb.gx + 1, C, R), _nan(gb.gx + 1, R, C), _nan(gb.gx + 1, R, C)
    dt, dtq = _nan(M, C, bf=True), _nan(M, C, bf=True)
    lib.call("mny_gate_bwd1_bf16", _p(y3), _p(d["s3"]), _p(d["b3"]), _p(dout), _p(wq), _p(d["sc1"]), _p(d["sh1"]), _p(d["sc2"]), _p(d["sh2"]),
             _p(d["mean2"]), _p(d["invstd2"]), _p(red2), M, C, R, _st())
    lib.call("mny_gate_bwd2_bf16", _p(y3), _p(d["s3"]), _p(d["b3"]), _p(dout), _p(wq), _p(d["sc1"]), _p(d["sh1"]), _p(d["mean1"]), _p(d["invstd1"]),
             _p(d["sc2"]), _p(d["sh2"]), _p(d["coef2"]), _p(red1), _p(dw2p), M, C, R, _st())
    with_red3 = lib.query("mny_gate_bwd_red3_supported", C, R) == 1
    assert with_red3 == (C != 160)
    lib.call("mny_gate_bwd3_bf16", _p(y3), _p(d["s3"]), _p(d["b3"]), _p(dout), _p(wq), _p(d["sc1"]), _p(d["sh1"]), _p(d["sc2"]), _p(d["sh2"]),
             _p(d["coef2"]), _p(d["coef1"]), None, None, _p(dt), _p(dw1p), None, M, C, R, _st())
    if with_red3:
        red3 = _nan(gb.gx + 1, 2, C)
        lib.call("mny_gate_bwd3_bf16", _p(y3), _p(d["s3"]), _p(d["b3"]), _p(dout), _p(wq), _p(d["sc1"]), _p(d["sh1"]), _p(d["sc2"]), _p(d["sh2"]),
                 _p(d["coef2"]), _p(d["coef1"]), _p(d["mean3"]), _p(d["invstd3"]), _p(dtq), _p(dw1q), _p(red3), M, C, R, _st())
    torch.cuda.synchronize()
    t2 = time.time()
    _same(_rows_written(st1, gf.gx, "stats1"), want["st1"], "sum, sum of squares of W1 t")
    _same(_rows_written(st2, gf.gx, "stats2"), want["st2"], "sum, sum of squares of W2 h")
    for kind in ge.RESIDUALS:
        _same(_host(outs[kind]), want["out:%s" % kind], "out (residual operand: %s)" % kind)
    _same(_rows_written(red2, gb.gx, "bwd1 sums"), want["red2"], "BN2 backward sums")
    _same(_rows_written(red1, gb.gx, "bwd2 sums"), want["red1"], "BN1 backward sums")
    _same(_rows_written(dw2p, gb.gx, "dW2 partials"), want["dw2"], "dW2")
    _same(_rows_written(dw1p, gb.gx, "dW1 partials"), want["dw1"], "dW1")
    _same(_host(dt), want["dt"], "dt")
    if with_red3:
        _same(_rows_written(dw1q, gb.gx, "dW1 partials (red3 form)"), want["dw1"], "dW1 (red3 form)")
        _same(_host(dtq), want["dt"], "dt (red3 form)")
        _same(_rows_written(red3, gb.gx, "red3"), want["red3"], "the project unit's BN backward sums over the stored dt")
    print("%s: fwd %d workgroups x %d trips (%d idle waves in the last iteration), bwd %d x %d (%d idle, %d pixels in the last tile): equal; "
          "reference %.2f s, GPU %.2f s, compare %.2f s, total %.2f s" % (r.id, gf.gx, gf.trips, gf.last_idle, gb.gx, gb.trips, gb.last_idle, gb.last_pixels,
                                                                         t1 - t0, t2 - t1, time.time() - t2, time.time() - t0))


@pytest.mark.parametrize("r", _ids(gr.PJ_TABLE))
def test_pj16_is_exact(lib, r):
    """mny_pj_bwd_bf16: gd, the partial rows of the sums and of dW, and the combined dW (the library's fp64 combine of the rows, rounded once to fp32);
    then once more with dw == NULL, where the partial rows must still be written."""
    t0 = time.time()
    g = _regime(lib, r)["bwd"]
    M, Ki, No = r.M, r.Ki, r.No
    assert lib.query("mny_pj_bwd_supported_bf16", M, Ki, No, r.act) == 1
    c = ge.pj_case(M, Ki, No, r.act)
    want = ge.pj_ref(c)[0]
    t1 = time.time()
    G, Y, D = (_dev(c[k], bf=True) for k in ("G", "Y", "D"))
    f = {k: _dev(c[k]) for k in ("coef", "d_scale", "d_shift", "d_mean", "d_invstd", "W")}
    got = []
    for with_dw in (True, False):
        gd, dw, dws, red = _nan(M, Ki, bf=True), _nan(No, Ki), _nan(g.gx + 1, No * Ki), _nan(g.gx + 1, 2, Ki)
        lib.call("mny_pj_bwd_bf16", _p(G), _p(Y), _p(f["coef"]), _p(D), _p(f["d_scale"]), _p(f["d_shift"]), _p(f["d_mean"]), _p(f["d_invstd"]), r.act,
                 _p(f["W"]), _p(gd), _p(dw) if with_dw else None, _p(dws), _p(red), M, Ki, No, _st())
        got.append((gd, dw, dws, red))
    torch.cuda.synchronize()
    t2 = time.time()
    for with_dw, (gd, dw, dws, red) in zip((True, False), got):
        tag = "" if with_dw else " (dw == NULL)"
        _same(_host(gd), want["gd"], "gd" + tag)
        _same(_rows_written(red, g.gx, "pj16 sums" + tag), want["red"], "sum dz, sum dz d_hat" + tag)
        _same(_rows_written(dws, g.gx, "pj16 dW partials" + tag).view(No, Ki), want["dw"], "dW partial rows" + tag)
        if with_dw:
            _same(_host(dw), ge.f32(want["dw"]), "dW")
        else:
            assert torch.isnan(_host(dw)).all(), "dw was written by a call that passed NULL for it"
    print("%s (act %d): %d workgroups x %d trips (%d idle waves in the last iteration, %d pixels in the last tile): equal; reference %.2f s, GPU %.2f s, "
          "compare %.2f s, total %.2f s" % (r.id, r.act, g.gx, g.trips, g.last_idle, g.last_pixels, t1 - t0, t2 - t1, time.time() - t2, time.time() - t0))


def test_cutting_three_gates_in_one_launch_equals_three_launches(lib):
    """mny_gate_cut_batch_bf16 with grid (16, 3): every job's chunk buffer, byte for byte, is what a single-job launch gives"""
    g = torch.Generator().manual_seed(3)
    jobs = [((torch.randn(R, C, generator=g) * (2.0 / C) ** 0.5).cuda(), (torch.randn(C, R, generator=g) * (2.0 / R) ** 0.5).cuda()) for (C, R) in gr.GATE_SHAPES]
    together = _cut(lib, jobs)
    for (C, R), job, wq in zip(gr.GATE_SHAPES, jobs, together):
        alone, = _cut(lib, [job])
        assert wq.numel() == alone.numel() == 2 * (gr.cdiv(R, 16) * gr.cdiv(gr.cdiv(C, 16), 2) + gr.cdiv(C, 16) * gr.cdiv(gr.cdiv(R, 16), 2)) * 64 * 16
        assert torch.equal(wq, alone), "C = %d: the chunk buffer of a three-job launch differs from the single-job one" % C
        # a chunk holds bf16 values of the weights or zeros: no byte of the 0xff pre-fill survives as a NaN pattern
        assert not torch.isnan(wq.view(torch.bfloat16).float()).any()
