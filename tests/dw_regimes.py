"""Launch geometry of the depthwise entry points (csrc/dwconv.hip, csrc/dwbwd.hip, csrc/dwtile.hip), restated in pure Python: which kernel
form a call takes, how many workgroups the capped grid has, and how many trips of the persistent loop

    register forms:  for (strip = lb * ppb + pix; strip < nstrips; strip += gx * ppb)
    tile forms:      for (tile = lb; tile < ntiles; tile += gx)

each workgroup walks.  The restatement follows dw_geom / dwb_geom / dwb2_geom / dwb5_geom / dwt_geom / make_stencil_layout and the routing rules
dwt_use / dwt_fwd_use at their defaults (no MNY_* switch set); tests/test_dw_regimes_cpu.py holds it against the library's own part-count queries.

TABLE lists the shapes tests/test_gpu_dw_trips.py runs: "trips" rows start a third, ragged trip; "tall" rows of the tile forms have strips of
at least 2 (K + 1) rows, so the (K + 1)-row LDS ring wraps at least twice inside one strip, on more tiles than workgroups.
"""
from collections import namedtuple

K_DWT_CG = 16
MAX_PARTS = 1024
S2_DATA_GRID = 8192        # grid cap of the stride-2 data-gradient kernels (no part rows: no query)


def cdiv(a, b):
    return -(-a // b)


def _round8(want):
    return (want + 7) & ~7 if want > 8 else want


def _cap(resident, chunks):
    cap = max(resident // chunks, 1)
    return cap & ~7 if cap > 8 else cap


def stencil_layout(C, max_cgb=64):
    cg_total = C // 4
    chunks = cdiv(cg_total, max_cgb)
    cgb = cdiv(cg_total, chunks)
    ppb = max(256 // cgb, 1)
    return dict(cg_total=cg_total, chunks=chunks, cgb=cgb, ppb=ppb, threads=cgb * ppb)


Regime = namedtuple("Regime", "form kernel gx cap ppb chunks units units_per_trip trips ragged TH nHS last_strip_h nWT last_tile_w PT CG xcd")


def _reg(form, kernel, gx, cap, ppb, chunks, units, TH, nHS, rows, nWT=0, last_tile_w=0, PT=0, CG=0):
    upt = gx * ppb
    return Regime(form, kernel, gx, cap, ppb, chunks, units, upt, cdiv(units, upt), units % upt != 0, TH, nHS, rows - (nHS - 1) * TH, nWT, last_tile_w,
                  PT, CG, gx % 8 == 0)


def _strips(form, kernel, N, rows, cols, th_max, resident, L):
    """register forms: strips of TH rows over (N, columns); one thread = one strip of one channel group"""
    ns = cdiv(rows, th_max)
    TH = cdiv(rows, ns)
    nHS = cdiv(rows, TH)
    nstrips = N * cols * nHS
    cap = _cap(resident, L["chunks"])
    gx = min(_round8(cdiv(nstrips, L["ppb"])), cap)
    return _reg(form, kernel, gx, cap, L["ppb"], L["chunks"], nstrips, TH, nHS, rows)


def dw_geom(N, H, W, C, K, stride, mode=0):
    """dw_geom of dwconv.hip.  mode 0: forward / stride-1 data gradient (second-generation kernels), 1: weight gradient"""
    P = K // 2
    Ho, Wo = (H + 2 * P - K) // stride + 1, (W + 2 * P - K) // stride + 1
    v2 = mode == 0 or K == 5
    resident = (512 if K == 5 else 768) if v2 else MAX_PARTS
    kernel = ("dw%d_fwd_kernel" % K) if mode == 0 else ("dw5_wgrad_kernel" if K == 5 else "dw_slide_kernel")
    return _strips("register", kernel, N, Ho, Wo, 16, resident, stencil_layout(C))


def dwb_geom(N, H, W, C):
    return _strips("register", "dw_bnbwd_s1k3_kernel", N, H, W, 32, 768, stencil_layout(C))


def dwb2_geom(N, H, W, C):
    return _strips("register", "dw_bnbwd_s2k3_kernel", N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 16, 768, stencil_layout(C))


def dwb5_geom(N, H, W, C):
    cg_total = C // 2
    chunks = cdiv(cg_total, 64)
    cgb = cdiv(cg_total, chunks)
    L = dict(cg_total=cg_total, chunks=chunks, cgb=cgb, ppb=max(256 // cgb, 1))
    return _strips("register", "dw_bnbwd_s2k5_kernel", N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 16, 768, L)


def dwt_pick_cg(K, C, bf):
    if bf and K == 3 and C == 16:
        return 4
    if bf and K == 3 and C == 72:
        return 18
    return K_DWT_CG


def dwt_geom(N, H, W, C, K, bf, fwd=False):
    CPT = 4 if fwd else (2 if K == 5 else 4)
    R = K // 2
    cg_total = C // CPT
    CG = K_DWT_CG if fwd else dwt_pick_cg(K, C, bf)
    NC = 2 if K == 5 else 1
    chunks = cdiv(cg_total, CG)
    nwt = cdiv(W, (256 // CG) * NC)
    PT = max(cdiv(cdiv(W, nwt), NC), cdiv(64, CG))
    if PT * NC < 2 * R:
        PT = cdiv(2 * R, NC)
    PC = PT * NC
    nWT = cdiv(W, PC)
    cap = _cap(768, chunks)
    best, bTH = -1.0, H
    for ns in range(1, H + 1):
        TH = cdiv(H, ns)
        if TH < 2 * R and ns > 1:
            break
        tiles = N * cdiv(H, TH) * nWT
        rounds = tiles / cap
        effr = rounds if rounds <= 1.0 else rounds / cdiv(tiles, cap)
        score = effr * (TH / (TH + R))
        if score > best:
            best, bTH = score, TH
    TH = bTH
    nHS = cdiv(H, TH)
    ntiles = N * nHS * nWT
    gx = min(_round8(ntiles), cap, ntiles)
    return _reg("tile", "dwf_tile_kernel" if fwd else "dwb_tile_kernel", gx, cap, 1, chunks, ntiles, TH, nHS, H, nWT, W - (nWT - 1) * PC, PT, CG)


def dwt_use(K, bf, red, C):
    if K == 5:
        return True
    if K != 3 or not bf:
        return False
    if C in (16, 72):
        return not red
    if C < 120:
        return False
    cg = C // 4
    chunks = cdiv(cg, K_DWT_CG)
    if 4 * cg < 3 * chunks * K_DWT_CG:
        return False
    return (not red) or C <= 192


def dwt_fwd_use(K, stride, bf, C):
    if stride != 1 or K not in (3, 5) or C % 4:
        return False
    if not bf or C < 120 or K != 5:
        return False
    cg = C // 4
    chunks = cdiv(cg, K_DWT_CG)
    return 4 * cg >= 3 * chunks * K_DWT_CG


def dw_bwd_data_s2_geom(N, H, W, C, K):
    L = stencil_layout(C)
    nq = N * ((H + 1) // 2) * ((W + 1) // 2)
    gx = min(cdiv(nq, L["ppb"]), S2_DATA_GRID)
    return _reg("register", "dw_bwd_data_s2k%d_kernel" % K, gx, S2_DATA_GRID, L["ppb"], L["chunks"], nq, 1, (H + 1) // 2, (H + 1) // 2)


def regime(op, N, H, W, C, K, stride, bf16=False, with_producer_sums=False):
    """(N, H, W) is the INPUT of the depthwise convolution (for the gradients: the tensor dX has the shape of).
    op: fwd | bwd_data | bwd_weight | bnbwd | bnbwd_s2 | bnbwd_s2k5"""
    if op == "fwd":
        return dwt_geom(N, H, W, C, K, 1, True) if dwt_fwd_use(K, stride, bf16, C) else dw_geom(N, H, W, C, K, stride)
    if op == "bwd_data":            # stride 1: the forward kernel over dY with the flipped filter
        return dw_geom(N, H, W, C, K, 1) if stride == 1 else dw_bwd_data_s2_geom(N, H, W, C, K)
    if op == "bwd_weight":
        return dw_geom(N, H, W, C, K, stride, 1)
    if op == "bnbwd":
        assert stride == 1
        return dwt_geom(N, H, W, C, K, bf16) if dwt_use(K, bf16, with_producer_sums, C) else dwb_geom(N, H, W, C)
    if op == "bnbwd_s2":
        assert K == 3 and stride == 2
        return dwb2_geom(N, H, W, C)
    if op == "bnbwd_s2k5":
        assert K == 5 and stride == 2
        return dwb5_geom(N, H, W, C)
    raise ValueError(op)


def query_args(op, N, H, W, C, K, stride, bf16=False, with_producer_sums=False):
    """[(name of the library's part-count query, its arguments)] that must equal regime(...).gx; empty where the kernel writes no part rows"""
    if op == "fwd":
        q = [("mny_dw_stat_parts_x", (N, H, W, C, K, stride, 1 if bf16 else 0))]
        if not dwt_fwd_use(K, stride, bf16, C):
            q.append(("mny_dw_stat_parts", (N, H, W, C, K, stride)))
        return q
    if op == "bwd_data":
        return [("mny_dw_stat_parts", (N, H, W, C, K, 1))] if stride == 1 else []
    if op == "bwd_weight":
        return [("mny_dw_wgrad_parts", (N, H, W, C, K, stride))]
    if op == "bnbwd":
        q = [("mny_dw_bnbwd_parts_k", (N, H, W, C, K, (1 if bf16 else 0) | (2 if with_producer_sums else 0)))]
        if K == 3 and not bf16 and not with_producer_sums:
            q.append(("mny_dw_bnbwd_parts", (N, H, W, C)))
        return q
    if op == "bnbwd_s2":
        return [("mny_dw_bnbwd_s2_parts", (N, H, W, C))]
    if op == "bnbwd_s2k5":
        return [("mny_dw_bnbwd_s2k5_parts", (N, H, W, C))]
    raise ValueError(op)


Row = namedtuple("Row", "id kind op N H W C K stride bf16 red")


def _r(id, kind, op, N, H, W, C, K, stride, bf16=False, red=False):
    return Row(id, kind, op, N, H, W, C, K, stride, bf16, red)


# kind "trips": the grid is at its cap and a third, ragged trip starts.  kind "tall" (tile forms): TH >= 2 (K + 1) and more tiles than workgroups.
# kind "small": at most 8 workgroups and not 8 of them — the only grids whose workgroups are NOT renumbered across the XCDs (a capped grid is a
# multiple of 8 by construction), one trip.
TABLE = [
    # second-generation forward (dw3_fwd_kernel / dw5_fwd_kernel): 768 / 512 resident workgroups over 4 channel chunks
    _r("fwd-k3s1", "trips", "fwd", 5, 5, 320, 960, 3, 1),
    _r("fwd-k3s2", "trips", "fwd", 8, 5, 386, 960, 3, 2),
    _r("fwd-k5s1", "trips", "fwd", 10, 5, 107, 960, 5, 1),
    _r("fwd-k5s2", "trips", "fwd", 10, 5, 213, 960, 5, 2),
    _r("fwd-k3s1-bf16", "trips", "fwd", 5, 5, 320, 960, 3, 1, True),
    # data gradient.  Stride 1: the forward kernel over dY with the flipped filter and an addend.  Stride 2: one thread per input quad on a grid capped at
    # 8192 workgroups, which 4 channels (256 quads per workgroup) reach at the fewest elements
    _r("bwd_data-k3s1", "trips", "bwd_data", 5, 5, 320, 960, 3, 1),
    _r("bwd_data-k5s1", "trips", "bwd_data", 10, 5, 107, 960, 5, 1),
    _r("bwd_data-k3s1-bf16", "trips", "bwd_data", 5, 5, 320, 960, 3, 1, True),
    _r("bwd_data-k3s2", "trips", "bwd_data", 3, 2049, 2735, 4, 3, 2),
    _r("bwd_data-k5s2", "trips", "bwd_data", 3, 2049, 2735, 4, 5, 2),
    # weight gradient: 3x3 on the sliding-window kernel (1024 / 4 workgroups), 5x5 on dw5_wgrad_kernel (512 / 4)
    _r("bwd_weight-k3", "trips", "bwd_weight", 20, 5, 107, 960, 3, 1),
    _r("bwd_weight-k5", "trips", "bwd_weight", 10, 5, 107, 960, 5, 1),
    _r("bwd_weight-k5s2", "trips", "bwd_weight", 10, 5, 213, 960, 5, 2),
    _r("bwd_weight-k5-bf16", "trips", "bwd_weight", 10, 5, 107, 960, 5, 1, True),
    # fused unit backward, register form (3x3 stride 1; on bf16 storage 960 channels stay on it only with producer sums)
    _r("bnbwd-k3", "trips", "bnbwd", 15, 5, 107, 960, 3, 1),
    _r("bnbwd-k3-red", "trips", "bnbwd", 15, 5, 107, 960, 3, 1, False, True),
    _r("bnbwd-k3-bf16-red", "trips", "bnbwd", 15, 5, 107, 960, 3, 1, True, True),
    # fused stride-2 units
    _r("bnbwd_s2", "trips", "bnbwd_s2", 24, 5, 213, 576, 3, 2),
    _r("bnbwd_s2-bf16", "trips", "bnbwd_s2", 24, 5, 213, 576, 3, 2, True),
    _r("bnbwd_s2k5", "trips", "bnbwd_s2k5", 10, 5, 213, 672, 5, 2),
    _r("bnbwd_s2k5-red", "trips", "bnbwd_s2k5", 10, 5, 213, 672, 5, 2, False, True),
    _r("bnbwd_s2k5-bf16-red", "trips", "bnbwd_s2k5", 10, 5, 213, 672, 5, 2, True, True),
    # tile backward
    _r("tile-k5-f32", "trips", "bnbwd", 13, 13, 33, 960, 5, 1),
    _r("tile-k5-bf16", "trips", "bnbwd", 13, 13, 33, 960, 5, 1, True),
    _r("tile-k5-bf16-red", "trips", "bnbwd", 13, 13, 33, 960, 5, 1, True, True),
    _r("tile-k3-bf16-cg16", "trips", "bnbwd", 17, 19, 33, 480, 3, 1, True),
    _r("tile-k3-bf16-c72", "trips", "bnbwd", 129, 19, 33, 72, 3, 1, True),
    _r("tile-k5-tall", "tall", "bnbwd", 41, 16, 11, 960, 5, 1, True),
    _r("tile-k3-tall", "tall", "bnbwd", 145, 9, 5, 480, 3, 1, True),
    # tile forward
    _r("tilefwd-k5", "trips", "fwd", 17, 13, 33, 960, 5, 1, True),
    _r("tilefwd-k5-tall", "tall", "fwd", 73, 12, 8, 960, 5, 1, True),
    # one small grid per kernel
    _r("small-dw3_fwd", "small", "fwd", 1, 6, 7, 960, 3, 1),
    _r("small-dw5_fwd", "small", "fwd", 1, 6, 7, 960, 5, 1),
    _r("small-dw_slide", "small", "bwd_weight", 1, 6, 7, 960, 3, 1),
    _r("small-dw5_wgrad", "small", "bwd_weight", 1, 6, 7, 960, 5, 1),
    _r("small-bwd_data-k3s2", "small", "bwd_data", 1, 6, 7, 960, 3, 2),
    _r("small-bwd_data-k5s2", "small", "bwd_data", 1, 6, 7, 960, 5, 2),
    _r("small-bnbwd-k3", "small", "bnbwd", 1, 6, 7, 960, 3, 1, False, True),
    _r("small-bnbwd_s2", "small", "bnbwd_s2", 1, 6, 14, 576, 3, 2),
    _r("small-bnbwd_s2k5", "small", "bnbwd_s2k5", 1, 6, 14, 672, 5, 2, False, True),
    _r("small-tile-k5", "small", "bnbwd", 3, 6, 7, 960, 5, 1, True, True),
    _r("small-tilefwd-k5", "small", "fwd", 3, 6, 7, 960, 5, 1, True),
]
