"""Launch geometry of the kernels of csrc/gate.hip that share the "a wave owns 16 pixels and all channels" machinery, restated in pure Python:

    gate_fwd_kernel<C, R, 1 | 2 | 3>:   4 waves;  for (tile = blockIdx.x * 4 + wave; tile < ntiles; tile += gridDim.x * 4)           grid capped at 512
    gate_bwd_kernel<C, R, 1 | 2 | 3>:   8 waves;  for (it = blockIdx.x; it < niter; it += gridDim.x), wave tile = it * 8 + wave       grid capped at 256
    pj16_bwd_kernel<KI, NO>:            8 waves;  the same loop, with the rows of iteration it + gridDim.x requested one trip ahead    grid capped at 512

A workgroup ITERATION is one pass of all its waves: 64 pixels forward, 128 backward.  The backward kernels keep barriers inside the loop, so every wave
of a workgroup runs every iteration of it: a wave whose tile lies past M ("idle") and the lanes of the last tile past M ("tail") read row 0 instead and
are masked with vm = 0.  Pass 2 / 3 of the gate and pj16 park both operands of the weight gradient transposed in LDS, 16 columns per wave; an idle wave
must overwrite its columns with zeros, or — when the iteration is a second or later trip of its workgroup — the previous trip's pixels are counted twice
(`stale_possible`).  tests/test_gate_regimes_cpu.py holds this restatement against mny_gate_parts, mny_gate_bwd_parts and mny_pj_bwd_parts_bf16.

TABLE lists the rows tests/test_gpu_gate_exact.py runs; every row names the regime it is there for (`want`), which the CPU test and the GPU test both
assert before anything runs.
"""
from collections import namedtuple

ACT_NONE, ACT_RELU6, ACT_LEAKY, ACT_RELU, ACT_HSWISH = 0, 1, 2, 3, 4
GATE_SHAPES = [(40, 10), (112, 28), (160, 40)]
PJ16_SHAPES = [(16, 16), (64, 24), (72, 24), (72, 40), (120, 40)]          # (Ki, No)
FWD_WAVES, FWD_CAP = 4, 512
BWD_WAVES, BWD_CAP = 8, 256
PJ_WAVES, PJ_CAP = 8, 512


def cdiv(a, b):
    return -(-a // b)


# gx: workgroups; tiles: 16-pixel wave tiles; iters: workgroup iterations in all; trips: of the busiest workgroup (workgroup 0); max_pixels: the most
# pixels one workgroup accumulates into its partial row (and its dW partial); last_*: the last iteration — the workgroup that runs it, which of that
# workgroup's trips it is (1-based), its live and idle waves, the pixels of its last live tile; stale_possible: last_trip >= 2
Regime = namedtuple("Regime", "form gx cap waves tiles iters trips max_pixels last_block last_trip last_live last_idle last_pixels stale_possible")


def _loop(form, M, waves, cap):
    assert M > 0
    tiles = cdiv(M, 16)
    iters = cdiv(tiles, waves)
    gx = min(iters, cap)
    per = 16 * waves
    # workgroup b walks iterations b, b + gx, ...: iteration `it` covers pixels [it * per, min(it * per + per, M))
    pixels = [sum(min(per, M - it * per) for it in range(b, iters, gx)) for b in {0, (iters - 1) % gx}]
    live = tiles - (iters - 1) * waves
    last_trip = (iters - 1) // gx + 1
    return Regime(form, gx, cap, waves, tiles, iters, cdiv(iters, gx), max(pixels), (iters - 1) % gx, last_trip, live, waves - live, M - (tiles - 1) * 16, last_trip >= 2)


def gate_grid(M):
    return _loop("gate_fwd_kernel", M, FWD_WAVES, FWD_CAP)


def gate_bwd_grid(M):
    return _loop("gate_bwd_kernel", M, BWD_WAVES, BWD_CAP)


def pj16_ok(M, Ki, No):
    return M >= 16 and (Ki, No) in PJ16_SHAPES


def pj16_grid(M, Ki, No):
    assert pj16_ok(M, Ki, No), (M, Ki, No)
    return _loop("pj16_bwd_kernel<%d,%d>" % (Ki, No), M, PJ_WAVES, PJ_CAP)


def pj16_flat(Ki):
    """Pj16Lds::flat: gd leaves through an LDS stage as whole 16-byte pieces (Ki >= 32) instead of straight from the accumulator layout"""
    return cdiv(Ki, 16) >= 2


def stale_pixels(g):
    """the pixels whose parked columns an idle wave of the last iteration would leave in LDS: those of the same waves one trip earlier"""
    if not g.stale_possible or g.last_idle == 0:
        return slice(0, 0)
    prev = g.iters - 1 - g.gx
    return slice((prev * g.waves + g.last_live) * 16, (prev + 1) * g.waves * 16)


def last_trip_start(g):
    """first pixel of the last trip of the whole grid (0 when there is one trip)"""
    return (g.trips - 1) * g.gx * g.waves * 16


def padding_group(n):
    """the last VALID group of four channels of a 16-channel tile that is only partly filled (None when n fills its tiles): a slice of channels"""
    if n % 16 == 0:
        return None
    return slice(4 * ((n - 1) // 4), n)


GateRow = namedtuple("GateRow", "id M C R want")
PjRow = namedtuple("PjRow", "id M Ki No act want")

# `want`: fwd / bwd -> fields of the regime the row is in the table for
_GATE_M = [
    # single partial tile: forward 3 idle waves, backward 7; every idle lane reads row 0
    ("g-one", 5, dict(fwd=dict(gx=1, tiles=1, trips=1, last_live=1, last_idle=3, last_pixels=5, stale_possible=False),
                      bwd=dict(gx=1, trips=1, last_live=1, last_idle=7, last_pixels=5, stale_possible=False))),
    # backward: 2 workgroups, the second with waves 0-1 full, wave 2 with 9 pixels, 5 idle; forward: 11 tiles on 3 workgroups, the last with 3
    ("g-wave", 169, dict(fwd=dict(gx=3, tiles=11, trips=1, last_block=2, last_live=3, last_idle=1, last_pixels=9),
                         bwd=dict(gx=2, iters=2, trips=1, last_block=1, last_live=3, last_idle=5, last_pixels=9, stale_possible=False))),
    # forward: 2058 tiles on 512 workgroups, the second trip covers 10 tiles, workgroup 2 has two live waves; backward: 258 iterations on 256
    # workgroups, iteration 257 is the second trip of workgroup 1 with 2 live waves (one of 3 pixels) and 6 idle
    ("g-trip2", 32915, dict(fwd=dict(gx=512, tiles=2058, iters=515, trips=2, last_block=2, last_trip=2, last_live=2, last_idle=2, last_pixels=3),
                            bwd=dict(gx=256, iters=258, trips=2, last_block=1, last_trip=2, last_live=2, last_idle=6, last_pixels=3, stale_possible=True,
                                     max_pixels=256))),
    # workgroup 0 takes a third trip: iteration 512 has 2 live waves
    ("g-trip3", 65557, dict(fwd=dict(gx=512, trips=3, last_block=0, last_trip=3, last_live=2, last_pixels=5),
                            bwd=dict(gx=256, iters=513, trips=3, last_block=0, last_trip=3, last_live=2, last_idle=6, last_pixels=5, stale_possible=True,
                                     max_pixels=277))),
]
GATE_TABLE = [GateRow("%s-%d" % (i, C), M, C, R, w) for (i, M, w) in _GATE_M for (C, R) in GATE_SHAPES]

# activation of the depthwise unit in front: none / ReLU6 / ReLU / h-swish in turn, so every instantiation meets at least three of them (leaky's slope
# 0.1 is no fp32-exact number: it stays with tests/test_gpu_pjbwd.py)
_PJ_ACTS = [ACT_NONE, ACT_RELU6, ACT_RELU, ACT_HSWISH]
_PJ_M = [
    ("p-min", 16, dict(gx=1, trips=1, last_live=1, last_idle=7, last_pixels=16, stale_possible=False)),
    ("p-wave", 169, dict(gx=2, trips=1, last_block=1, last_live=3, last_idle=5, last_pixels=9, stale_possible=False)),
    # 514 iterations on 512 workgroups: iteration 513 is the second trip of workgroup 1, 2 live waves, the last with 3 pixels; workgroups 2 .. 511
    # request the rows of an iteration past the last one
    ("p-trip2", 65683, dict(gx=512, iters=514, trips=2, last_block=1, last_trip=2, last_live=2, last_idle=6, last_pixels=3, stale_possible=True, max_pixels=256)),
    # a third trip, ragged: for the store straight from the accumulators (16,16) and the staged one (72,24)
    ("p-trip3", 131093, dict(gx=512, iters=1025, trips=3, last_block=0, last_trip=3, last_live=2, last_idle=6, last_pixels=5, stale_possible=True, max_pixels=277)),
]
PJ_TRIP3 = [(16, 16), (72, 24)]
PJ_TABLE = []
for (_Ki, _No) in PJ16_SHAPES:
    for (_i, _M, _w) in _PJ_M:
        if _i == "p-trip3" and (_Ki, _No) not in PJ_TRIP3:
            continue
        PJ_TABLE.append(PjRow("%s-%d-%d" % (_i, _Ki, _No), _M, _Ki, _No, _PJ_ACTS[len(PJ_TABLE) % 4], _w))

TABLE = GATE_TABLE + PJ_TABLE


def regimes(r):
    """{pass family: Regime} of a table row"""
    if isinstance(r, PjRow):
        return {"bwd": pj16_grid(r.M, r.Ki, r.No)}
    return {"fwd": gate_grid(r.M), "bwd": gate_bwd_grid(r.M)}


def queries(r):
    """[(query name, arguments, expected value)] of the library that a row's restated geometry must match"""
    if isinstance(r, PjRow):
        return [("mny_pj_bwd_parts_bf16", (r.M, r.Ki, r.No), pj16_grid(r.M, r.Ki, r.No).gx)]
    return [("mny_gate_parts", (r.M,), gate_grid(r.M).gx), ("mny_gate_bwd_parts", (r.M,), gate_bwd_grid(r.M).gx)]


def check_regime(r):
    """assert that the row is in the regime its `want` claims; returns regimes(r)"""
    gs = regimes(r)
    want = {"bwd": r.want} if isinstance(r, PjRow) else r.want
    for fam, w in want.items():
        g = gs[fam]
        for k, v in w.items():
            assert getattr(g, k) == v, "%s %s: %s is %r, the table claims %r (%r)" % (r.id, fam, k, getattr(g, k), v, g)
        assert g.last_live + g.last_idle == g.waves and 1 <= g.last_pixels <= 16 and g.stale_possible == (g.last_trip >= 2), (r.id, g)
        if g.trips >= 2:
            assert g.gx == g.cap and g.last_trip == g.trips, (r.id, g)
    return gs
