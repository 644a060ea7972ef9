"""Launch geometry of the kernels at the two ends of a block (csrc/stem.hip, csrc/stemdw.hip, the fp32 csrc/pjbwd.hip), restated in pure Python:
which kernel form a call takes, how many workgroups the capped grid has, and how many trips of the persistent loop

    stem_tile_kernel / stem_wgrad_mfma_kernel / stemdw_bwd_kernel:  for (tile = lb; tile < ntiles; tile += gx)
    stem_kernel:                                                    for (p = blockIdx.x * ppb + pix; p < npix; p += gx * ppb)
    pj_bwd_kernel:                                                  for (t = blockIdx.x * 4 + wave; t < ntiles; t += gx * 4)

each workgroup walks.  The restatement follows stem_geom / stem_mfma_grid / sd_geom / pj_grid at default switches; MNY_STEM_WGRAD_VALU is latched
by the library at its first use, so it is read from the process's environment here and never flipped.  tests/test_stem_regimes_cpu.py holds the
restatement against the library's own part-count queries.

TABLE lists the shapes tests/test_gpu_stem_trips.py runs; every row names the regime it is there for (`want`), which the CPU test and the GPU test
both assert before anything runs.
"""
import os
from collections import namedtuple

ST_TH, ST_TW = 8, 32                      # stem tile: 8 x 32 output pixels
SD_OWN, SD_C, SD_K = 30, 32, 27           # stemdw: 30 owned columns per workgroup; Cout; taps
SD_STRIDE = SD_C * SD_K + SD_K * SD_K + 2 * SD_C + SD_K            # bnw_stride(32, 27): [P1 | Gram | s1 | s2 | colsum]
ACT_NONE, ACT_RELU6, ACT_LEAKY, ACT_RELU, ACT_HSWISH = 0, 1, 2, 3, 4


def cdiv(a, b):
    return -(-a // b)


def out_hw(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def valu_switch():
    return os.environ.get("MNY_STEM_WGRAD_VALU", "") not in ("", "0")


# form: the kernel (and its MODE); gx: workgroups; units: tiles (stem_kernel: pixels) in all; units_per_trip: what one trip of the whole grid covers;
# trips: of the busiest workgroup; ragged: the last trip does not fill the grid; last_units: units in the last trip; last_h, last_w: size of the last
# unit (pixels of the last 16-pixel tile x 1 for pj; 1 x 1 for stem_kernel); staging: how a stem tile's image patch is loaded; xcd: workgroups renumbered
Regime = namedtuple("Regime", "form gx cap units units_per_trip trips ragged last_units last_h last_w staging xcd extra")


def _reg(form, gx, cap, units, upt, last_h, last_w, staging="", xcd=False, **extra):
    trips = cdiv(units, upt)
    return Regime(form, gx, cap, units, upt, trips, units % upt != 0, units - (trips - 1) * upt, last_h, last_w, staging, xcd, extra)


def stem_tiled_ok(Cout):
    cgn = Cout // 4
    return cgn > 0 and 256 % cgn == 0


def stem_mfma_ok(Cout):
    return not valu_switch() and Cout in (16, 32)


def stem_geom(op, N, H, W, Cout):
    """op: fwd (mny_stem_fwd) | wgrad (mny_stem_wgrad) | bnwgrad (mny_stem_bnwgrad)"""
    assert N > 0 and H > 0 and W > 0 and Cout % 4 == 0 and 4 <= Cout <= 256
    Ho, Wo = out_hw(H, W)
    cgb = Cout // 4
    mode = {"fwd": 0, "wgrad": 1, "bnwgrad": 2}[op]
    if not stem_tiled_ok(Cout):
        assert op != "bnwgrad", "mny_stem_bnwgrad_supported(%d) == 0" % Cout
        ppb = 256 // cgb
        npix = N * Ho * Wo
        gx = min(cdiv(npix, ppb), 768)
        return _reg("stem_kernel<%d>" % mode, gx, 768, npix, gx * ppb, 1, 1, "direct", cgn=cgb, ppb=ppb)
    th, tw = cdiv(Ho, ST_TH), cdiv(Wo, ST_TW)
    ntiles = N * th * tw
    staging = "float4" if W % 4 == 0 else "scalar"
    lh, lw = Ho - (th - 1) * ST_TH, Wo - (tw - 1) * ST_TW
    if op != "fwd" and stem_mfma_ok(Cout):
        cap = 768 if Cout == 16 else 512
        return _reg("stem_wgrad_mfma_kernel<%d>" % (mode - 1), min(ntiles, cap), cap, ntiles, min(ntiles, cap), lh, lw, staging, cgn=cgb, ppb=256 // cgb)
    return _reg("stem_tile_kernel<%d>" % mode, min(ntiles, 768), 768, ntiles, min(ntiles, 768), lh, lw, staging, cgn=cgb, ppb=256 // cgb)


def stem_query(op):
    return "mny_stem_stat_parts" if op == "fwd" else "mny_stem_wgrad_parts"


def sd_geom(N, H, W):
    assert N > 0 and H >= 8 and W >= 8
    Ho, Wo = out_hw(H, W)
    ns = cdiv(Ho, 32)
    TH = cdiv(Ho, ns)
    nHS = cdiv(Ho, TH)
    nWT = cdiv(Wo, SD_OWN)
    ntiles = N * nHS * nWT
    want = (ntiles + 7) & ~7 if ntiles > 8 else ntiles
    gx = min(want, 512)
    return _reg("stemdw_bwd_kernel", gx, 512, ntiles, gx, Ho - (nHS - 1) * TH, Wo - (nWT - 1) * SD_OWN, "", gx % 8 == 0, TH=TH, nHS=nHS, nWT=nWT, Ho=Ho, Wo=Wo)


def sd_first_tile(block, gx):
    """the tile workgroup `block` starts at: workgroups are renumbered across the 8 XCDs when the grid is a multiple of 8"""
    return (block & 7) * (gx >> 3) + (block >> 3) if gx % 8 == 0 else block


def sd_ws_floats(N, H, W):
    return (sd_geom(N, H, W).gx + 1) * SD_STRIDE + SD_C * SD_K + SD_K * SD_K + 64


def pj_grid(M, Ki, No):
    assert M >= 16 and No in (16, 24, 32) and Ki in (32, 96, 144, 192)
    ntiles = cdiv(M, 16)
    cap = 1024 if Ki == 32 else 512
    gx = max(min(cdiv(ntiles, 4), cap), 1)
    return _reg("pj_bwd_kernel<%d,%d>" % (No, Ki), gx, cap, ntiles, 4 * gx, M - (ntiles - 1) * 16, 1, "", False, prefetch=Ki // 16 <= 6)


SdRow = namedtuple("SdRow", "id N H W want")
StRow = namedtuple("StRow", "id N H W Cout want")
PjRow = namedtuple("PjRow", "id M Ki No act want")

# `want`: properties of the regime the row is in the table for (checked by check_regime below)
SD_TABLE = [
    SdRow("sd-trips", 1100, 9, 9, dict(units=1100, gx=512, trips=3, ragged=True, xcd=True, last_h=5, last_w=5, TH=5, nHS=1, nWT=1, odd="HW")),
    SdRow("sd-strips", 90, 67, 125, dict(units=540, gx=512, trips=2, ragged=True, xcd=True, Ho=34, TH=17, nHS=2, Wo=63, nWT=3, last_w=3, odd="HW")),
    SdRow("sd-min-8x8", 3, 8, 8, dict(units=3, gx=3, trips=1, xcd=False, odd="")),
    SdRow("sd-min-9x8", 2, 9, 8, dict(units=2, gx=2, trips=1, xcd=False, odd="H")),
    SdRow("sd-min-8x9", 2, 8, 9, dict(units=2, gx=2, trips=1, xcd=False, odd="W")),
    SdRow("sd-edge30", 3, 61, 59, dict(Wo=30, nWT=1, last_w=30, Ho=31, nHS=1, trips=1, odd="HW")),
    SdRow("sd-edge1-63x121", 2, 63, 121, dict(Wo=61, nWT=3, last_w=1, trips=1, odd="HW")),
    SdRow("sd-edge1-129x61", 5, 129, 61, dict(Ho=65, TH=22, nHS=3, last_h=21, Wo=31, nWT=2, last_w=1, units=30, gx=32, trips=1, xcd=True, odd="HW")),
]

# per op: fwd / wgrad / bnwgrad.  `mfma` wants hold at default switches (MNY_STEM_WGRAD_VALU unset); with the switch the vector-ALU forms run instead
ST_TABLE = [
    StRow("st-trips32", 1100, 15, 15, 32, dict(units=1100, last_h=8, last_w=8, staging="scalar", ragged=True,
                                               fwd=dict(form="stem_tile_kernel<0>", gx=768, trips=2), mfma=dict(gx=512, trips=3), valu=dict(gx=768, trips=2))),
    StRow("st-trips16", 1600, 15, 15, 16, dict(units=1600, last_h=8, last_w=8, staging="scalar", ragged=True,
                                               fwd=dict(form="stem_tile_kernel<0>", gx=768, trips=3), mfma=dict(gx=768, trips=3), valu=dict(gx=768, trips=3))),
    StRow("st-valu64", 900, 15, 17, 64, dict(units=900, staging="scalar", ragged=True, fwd=dict(form="stem_tile_kernel<0>", gx=768, trips=2),
                                             valu=dict(gx=768, trips=2), cgn=16)),
    StRow("st-valu8", 1700, 15, 13, 8, dict(units=1700, staging="scalar", ragged=True, last_w=7, fwd=dict(form="stem_tile_kernel<0>", gx=768, trips=3),
                                            valu=dict(gx=768, trips=3), cgn=2)),
    StRow("st-odd", 3, 101, 133, 32, dict(w_mod4=1, last_h=3, last_w=3, staging="scalar", fwd=dict(form="stem_tile_kernel<0>", trips=1), mfma=dict(trips=1), valu=dict(trips=1))),
    StRow("st-odd4", 3, 101, 132, 16, dict(w_mod4=0, last_h=3, staging="float4", fwd=dict(form="stem_tile_kernel<0>", trips=1), mfma=dict(trips=1), valu=dict(trips=1))),
    StRow("st-oddH1", 2, 33, 35, 64, dict(last_h=1, staging="scalar", fwd=dict(form="stem_tile_kernel<0>", trips=1), valu=dict(trips=1))),
    StRow("st-plain-21x27", 2, 21, 27, 12, dict(staging="direct", fwd=dict(form="stem_kernel<0>", trips=1), valu=dict(form="stem_kernel<1>", trips=1))),
    StRow("st-plain-17x15", 40, 17, 15, 12, dict(staging="direct", fwd=dict(form="stem_kernel<0>", trips=1), valu=dict(form="stem_kernel<1>", trips=1))),
]

# activation of the unit in front: none / ReLU6 / leaky / ReLU, three rows each
_PJ_ACTS = [ACT_NONE, ACT_RELU6, ACT_LEAKY, ACT_RELU]
PJ_TABLE = []
for _i, (_No, _Ki) in enumerate((no, ki) for no in (16, 24, 32) for ki in (32, 96, 144, 192)):
    _M = 131155 if _Ki == 32 else 65619
    PJ_TABLE.append(PjRow("pj-%d-%d" % (_No, _Ki), _M, _Ki, _No, _PJ_ACTS[(_i + _i // 4) % 4],
                          dict(units=8198 if _Ki == 32 else 4102, gx=1024 if _Ki == 32 else 512, trips=3, ragged=True, last_units=6, last_h=3, prefetch=_Ki <= 96)))

TABLE = SD_TABLE + ST_TABLE + PJ_TABLE

# the (No, Ki) instantiations of pj_bwd_kernel no kernel test launched before this table
PJ_NEVER_LAUNCHED = {(16, 96), (16, 144), (16, 192), (24, 32), (24, 192), (32, 32), (32, 96)}

STEM_OPS = ("fwd", "wgrad", "bnwgrad")


def stem_ops(r):
    return [op for op in STEM_OPS if op != "bnwgrad" or stem_tiled_ok(r.Cout)]


def regimes(r):
    """{op: Regime} of a table row"""
    if isinstance(r, SdRow):
        return {"bwd": sd_geom(r.N, r.H, r.W)}
    if isinstance(r, PjRow):
        return {"bwd": pj_grid(r.M, r.Ki, r.No)}
    return {op: stem_geom(op, r.N, r.H, r.W, r.Cout) for op in stem_ops(r)}


def queries(r):
    """[(query name, arguments, expected value)] of the library that a row's restated geometry must match"""
    if isinstance(r, SdRow):
        return [("mny_stemdw_bwd_parts", (r.N, r.H, r.W, SD_C), sd_geom(r.N, r.H, r.W).gx), ("mny_stemdw_bwd_ws_floats", (r.N, r.H, r.W, SD_C), sd_ws_floats(r.N, r.H, r.W))]
    if isinstance(r, PjRow):
        return [("mny_pj_bwd_parts", (r.M, r.Ki, r.No), pj_grid(r.M, r.Ki, r.No).gx)]
    return [(stem_query(op), (r.N, r.H, r.W, r.Cout), g.gx) for op, g in regimes(r).items()]


def _holds(g, want, what):
    for k, v in want.items():
        got = getattr(g, k) if k in Regime._fields else g.extra[k]
        assert got == v, "%s: %s is %r, the table claims %r (%r)" % (what, k, got, v, g)


def check_regime(r):
    """assert that the row is in the regime its `want` claims; returns regimes(r)"""
    gs = regimes(r)
    want = dict(r.want)
    if isinstance(r, StRow):
        per = {k: want.pop(k, {}) for k in ("fwd", "mfma", "valu")}
        w4 = want.pop("w_mod4", None)
        assert w4 is None or r.W % 4 == w4, r.id
        assert r.H % 2 == 1 and (r.W % 2 == 1 or w4 == 0), r.id + ": an odd size is the point of every stem row"
        for op, g in gs.items():
            w = dict(want)
            if g.form.startswith("stem_kernel"):
                w.pop("last_h", None), w.pop("last_w", None)
            w.update(per["fwd"] if op == "fwd" else per["mfma"] if g.form.startswith("stem_wgrad_mfma") else per["valu"])
            if op != "fwd" and not g.form.startswith("stem_wgrad_mfma") and "form" not in w:
                w["form"] = "stem_tile_kernel<%d>" % (1 if op == "wgrad" else 2)
            _holds(g, w, "%s %s" % (r.id, op))
            if w.get("trips", 1) >= 2:
                assert g.gx == g.cap and g.ragged, (r.id, op, g)
        return gs
    g = gs["bwd"]
    if isinstance(r, SdRow):
        odd = want.pop("odd")
        assert (r.H % 2 == 1) == ("H" in odd) and (r.W % 2 == 1) == ("W" in odd), r.id
    _holds(g, want, r.id)
    if want.get("trips", 1) >= 2:
        assert g.gx == g.cap and g.units > (want["trips"] - 1) * g.units_per_trip, (r.id, g)
    return gs


def unit_pixels(r, op, unit):
    """the output pixels of unit `unit` of a row's kernel as (n, row slice, column slice) of [N, Ho, Wo] (stem tile forms, stemdw) or as a slice of the
    flattened pixels (stem_kernel, pj)"""
    g = regimes(r)[op]
    if isinstance(r, PjRow):
        return slice(16 * unit, min(16 * unit + 16, r.M))
    if isinstance(r, SdRow):
        e = g.extra
        wt, hs, n = unit % e["nWT"], (unit // e["nWT"]) % e["nHS"], unit // (e["nWT"] * e["nHS"])
        return n, slice(hs * e["TH"], min(hs * e["TH"] + e["TH"], e["Ho"])), slice(wt * SD_OWN, min(wt * SD_OWN + SD_OWN, e["Wo"]))
    if g.form.startswith("stem_kernel"):
        return slice(unit, unit + 1)
    Ho, Wo = out_hw(r.H, r.W)
    th, tw = cdiv(Ho, ST_TH), cdiv(Wo, ST_TW)
    c, rr, n = unit % tw, (unit // tw) % th, unit // (tw * th)
    return n, slice(rr * ST_TH, min(rr * ST_TH + ST_TH, Ho)), slice(c * ST_TW, min(c * ST_TW + ST_TW, Wo))
