"""tests/wgrad_regimes.py (the plan and the route of the weight-gradient tile kernels, restated) and tests/wgrad_exact_ref.py (the exact inputs) held
against the library's host queries, the sources and themselves — no GPU:

  * the restatement gives mny_pw_wgrad_splits[_bf16], mny_pw_wgrad_kernel and mny_pw_route(2, ...) over a sweep of (M, K, N, type, view, bias);
    mny_pw_wgrad_ws_floats holds the partial rows of either storage type;
  * ROWS is the list of instantiations the sources compile (the per-tile macro lists `X(MD, I, J)` and the six-product cases, wherever under csrc/ they live);
  * TABLE reaches every element of ROWS — a missing instantiation fails by name — and every row is in the regime it declares;
  * the inputs of every table row are exact: representable where a kernel rounds, every split's sum of |products| below 2^24 units, no dead row
    inside a 32-channel block;
  * three modelled faults, per template: equality sees each, and the test prints whether the relative-to-maximum bound of the older tests would
    have;
  * how many of the 113 instantiations the direct calls of the older tests reach (printed; pinned).
"""
import glob
import os
import re

import numpy as np
import pytest
import torch

import wgrad_exact_ref as we
import wgrad_regimes as wr

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "mobilenet-yolo-pytorch_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    from mobilenet_yolo_pytorch_amd import _lib
    _lib.load()
    return _lib


SWEEP_M = [1, 5, 17, 64, 65, 193, 385, 769, 1000, 4097, 4166, 8200, 16384, 16400, 30976, 123904, 200000]
SWEEP_C = [1, 3, 4, 8, 12, 20, 24, 32, 33, 36, 40, 64, 68, 72, 96, 100, 128, 132, 136, 160, 164, 168, 192, 196, 200, 256, 264, 320, 384, 512, 576, 960, 1280]
SWEEP_VIEWS = [(wr.ACT_NONE, False), (wr.ACT_RELU6, True), (wr.ACT_RELU, False), (wr.ACT_LEAKY, True), (wr.ACT_HSWISH, True), (wr.ACT_HSWISH, False)]


def test_restatement_matches_the_library(lib):
    n, codes = 0, set()
    for M in SWEEP_M:
        for K in SWEEP_C:
            for N in SWEEP_C:
                for bf in (0, 1):
                    plain = wr.route(bf, M, K, N)
                    sfx = "_bf16" if bf else ""
                    want_splits = plain.plan.splits if plain.plan else lib.query("mny_pw_wgrad_splits", M, K, N)
                    assert lib.query("mny_pw_wgrad_splits" + sfx, M, K, N) == want_splits, (bf, M, K, N)
                    assert lib.query("mny_pw_route", 2, bf, M, K, N) == plain.family, (bf, M, K, N)
                    for act, view in SWEEP_VIEWS:
                        for bias in (False, True):
                            r = wr.route(bf, M, K, N, act, view, bias)
                            assert lib.query("mny_pw_wgrad_kernel", bf, M, K, N, act, int(view), int(bias)) == r.code, (bf, M, K, N, act, view, bias, r)
                            codes.add((bf, r.code, r.xf if r.inst is not None and r.inst.template == wr.T_BF16 else 0))
                            n += 1
                    # the workspace holds the partial rows of the fp32 call with and without a bias gradient and of the bf16 call (which has no
                    # query of its own: K 96, N 200 plans twice the splits in bf16) — and the column sums behind them
                    need = max(want_splits, wr.route(0, M, K, N, bias=True).plan.splits, lib.query("mny_pw_wgrad_splits_bf16", M, K, N))
                    assert lib.query("mny_pw_wgrad_ws_floats", M, K, N) >= need * N * K + min(wr.cdiv(M, 256), 512) * N, (M, K, N)
    print("restatement == library at %d calls, %d distinct kernels" % (n, len(codes)))


def test_kernel_query_needs_no_gpu_and_rejects_an_empty_problem(lib):
    L = lib.load()
    for args in ((0, 0, 8, 8), (1, 5, 0, 8), (0, 5, 8, -1)):
        assert L.mny_pw_wgrad_kernel(args[0], args[1], args[2], args[3], 0, 0, 0) == -1
    # the six-product route on a MODE 1 plan, and on a MODE 0 tile outside the five six-product ones, launches the fp32-MFMA kernel: template 1
    assert lib.query("mny_pw_route", 2, 0, 4100, 96, 576) == wr.ROUTE_DMA_X6 and lib.query("mny_pw_wgrad_kernel", 0, 4100, 96, 576, 0, 0, 0) == 1123
    assert lib.query("mny_pw_route", 2, 0, 1000, 68, 132) == wr.ROUTE_DMA_X6 and lib.query("mny_pw_wgrad_kernel", 0, 1000, 68, 132, 0, 0, 0) == 2012
    assert lib.query("mny_pw_wgrad_kernel", 0, 16384, 64, 384, 0, 0, 0) == 5000 and lib.query("mny_pw_wgrad_kernel", 0, 16384, 64, 384, 0, 0, 1) == 2021
    assert lib.query("mny_pw_wgrad_kernel", 0, 30976, 512, 512, 1, 1, 0) == 2024


def _sources():
    return "\n".join(open(f).read() for f in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h"))))


def test_rows_are_the_instantiations_the_sources_compile():
    src = _sources()
    found = []
    for m in re.finditer(r"#define (\w+)\(MD, I, J\)([^\n]*)\n(.*?)#undef \1\b", src, re.S):
        name, body, block = m.groups()
        tiles = [tuple(int(v) for v in t) for t in re.findall(r"\b%s\((\d), (\d), (\d)\)" % name, block)]
        assert tiles, body
        if "pw_wgrad_bf16_kernel" in body:
            xfs = sorted(int(v) for v in re.findall(r"pw_wgrad_bf16_kernel<MD, I, J, (\d)>", body))
            found += [wr.Inst(wr.T_BF16, "bf16", *t, xf) for t in tiles for xf in xfs]
        elif "pw_wgrad_dma_kernel<MD, I, J>" in body:
            found += [wr.Inst(wr.T_DMA, "f32", *t, 0) for t in tiles]
        elif "pw_wgrad_kernel<T, MD, I, J>" in body:
            types = sorted(set(re.findall(r"pw_wgrad_impl<(\w+)>\(", src)))
            assert types == ["bf16_t", "float"], types
            found += [wr.Inst(wr.T_REG, ty, *t, 0) for ty in ("f32", "bf16") for t in tiles]
    found += [wr.Inst(wr.T_X6, "f32", *(int(v) for v in t), 1) for t in re.findall(r"case \d+: return \(WgKernel\)pw_wgrad_dma_kernel<(\d), (\d), (\d), 1>;", src)]
    assert len(found) == len(set(found)), "an instantiation is listed twice"
    missing, extra = sorted(set(wr.ROWS) - set(found)), sorted(set(found) - set(wr.ROWS))
    assert not missing and not extra, ("ROWS only: %s; sources only: %s" % ([wr.inst_name(i) for i in missing], [wr.inst_name(i) for i in extra]))
    assert len(found) == 113


def test_table_reaches_every_instantiation_in_the_declared_regime():
    seen = {}
    for row in wr.TABLE:
        r, g = wr.check_regime(row)
        assert r.inst in wr.ROWS, row.id
        assert row.M <= wr.LIMIT_M and row.K <= wr.LIMIT_C and row.N <= wr.LIMIT_C, row.id
        seen.setdefault(r.inst, []).append((row, r, g))
    missing = [wr.inst_name(i) for i in wr.ROWS if i not in seen]
    assert not missing, "no table row launches %s" % ", ".join(missing)
    assert len({row.id for row in wr.TABLE}) == len(wr.TABLE)
    odd_k = odd_n = 0
    multi, no_multi = wr.multi_reachable(), []
    assert set(multi) <= set(wr.ROWS) and len(multi) == 32, len(multi)      # (every MODE 0 tile of every template and view; fp32 <1,2,3>, <1,3,2>)
    for inst, rows in seen.items():
        name = wr.inst_name(inst)
        wants = {w for row, _, _ in rows for w in row.want.split("+")}
        assert {"one", "two", "steady", "tail1"} <= wants, (name, wants)
        assert any(row.bias for row, _, _ in rows) and any(not row.bias for row, _, _ in rows), name
        tile = (inst.mode, inst.TI, inst.TJ)
        if tile != (0, 2, 4):                       # (the 128 x 256 tile needs K % 256 == 0 and N % 128 == 0)
            assert any(g.ragged_k and g.ragged_n for _, _, g in rows), name + ": no row ragged in K and N"
        # a grid of several workgroups per split wherever the RESTATEMENT finds one for the instantiation within the limits (not: wherever the table
        # happens to hold one): below 64 splits, and for the LDS-DMA kernels in XCD order with dead workgroups
        if inst in multi:
            need = {"grid3d"} if inst.template == wr.T_REG else {"grid3d", "xcd"}
            got = {w for row, _, g in rows if g.multi for w in row.want.split("+")}
            if not need <= got:
                no_multi.append("%s (e.g. K %d, N %d): rows %s missing" % ((name,) + multi[inst] + (sorted(need - got),)))
        else:
            assert not any(g.multi for _, _, g in rows), name
        views = {row.view for row, _, _ in rows}
        if inst.template in (wr.T_DMA, wr.T_X6):
            assert {"none", "bn6", "relu"} <= views, (name, views)
        if inst.template == wr.T_BF16:
            assert views <= {0: {"none"}, 1: {"bn6", "relu", "bn", "bnrelu", "leaky"}, 2: {"hs3", "hs"}}[inst.variant], (name, views)
        if inst.template == wr.T_REG:
            al = 8 if inst.type == "bf16" else 4
            assert any(row.K % al or row.N % al for row, _, _ in rows), name
            if inst.type == "f32":
                assert any(row.K % 4 == 0 and row.N % 4 == 0 and row.view in ("hs", "hs3") for row, _, _ in rows), name + ": no aligned h-swish row"
            odd_k += any(row.K % 2 for row, _, _ in rows)
            odd_n += any(row.N % 2 for row, _, _ in rows)
    assert odd_k >= 1 and odd_n >= 1
    assert not no_multi, "a plan with gx * gy > 1 exists but the table does not run it: " + "; ".join(no_multi)
    # the two 96-wide fp32 tiles on a grid of several workgroups, just above 64 splits of 128 rows; and the six-product family on a MODE 1 plan
    for tile in ((1, 2, 3), (1, 3, 2)):
        rows = [(row, r, g) for row, r, g in seen[wr.Inst(wr.T_DMA, "f32", *tile, 0)] if g.multi]
        assert any(g.xcd and g.splits == 65 and r.family == wr.ROUTE_DMA_X6 for row, r, g in rows), tile
    assert {row.view for row in wr.LEAKY_TABLE} == {"leaky"} and {wr.check_regime(row)[0].inst.template for row in wr.LEAKY_TABLE} == {0, 1, 2, 3}
    print("%d table rows for %d instantiations" % (len(wr.TABLE), len(seen)))


def _kinds(row):
    """the input classes a row runs: the 16-bit class only where a call without a view launches the row's own instantiation"""
    if row.bf16 or row.view == "leaky" or wr.route(0, row.M, row.K, row.N).inst != row.inst:
        return ["small"]
    return ["small", "wide16", "wide16-swapped"]


def _bf16_exact(t):
    return torch.equal(we.bf(t), t)


def test_inputs_of_every_table_row_are_exact():
    worst = 0.0
    for row in wr.EXACT_TABLE:
        r, g = wr.check_regime(row)
        for kind in _kinds(row):
            c = we.case(row, kind)
            a = we.activated(c)
            assert torch.equal(we.f32(c["X"]), c["X"]) and torch.equal(we.f32(c["dY"]), c["dY"]) and torch.equal(we.f32(a), a), row.id
            if kind == "small":
                # representable where a kernel rounds: bf16 storage of X and dY, the bf16 kernel's rounding of the activated operand, and the cut of the
                # six-product form (hi piece = the whole value)
                assert _bf16_exact(c["X"]) and _bf16_exact(c["dY"]) and _bf16_exact(a), row.id
                if c["scale"] is not None:
                    z = c["X"] * c["scale"] + c["shift"]
                    assert torch.equal(we.f32(z), z), row.id
                    if c["act"] == wr.ACT_HSWISH:
                        assert bool(((z <= -3) | (z == 0) | (z >= 3)).all()), row.id
                        z32 = z.to(torch.float32)          # the kernels' own expression in fp32 gives exactly 0 or z
                        hs = z32 * torch.clamp(z32 + 3, 0, 6) * np.float32(1.0 / 6.0)
                        assert torch.equal(hs.to(we.F64), a) and torch.equal((z32 * (torch.clamp(z32 + 3, 0, 6) * np.float32(1.0 / 6.0))).to(we.F64), a), row.id
            else:
                wide = c["X"] if kind == "wide16" else c["dY"]
                assert not _bf16_exact(wide) and bool((wide.abs() >= 2 ** 15).all()) and bool((wide.abs() < 2 ** 16).all()) and bool((wide % 2 == 1).all()), row.id
            units = we.worst_units(c, g, row.M)
            assert units < we.LIMIT, (row.id, kind, units)
            worst = max(worst, units)
            # every product is a whole number of units
            assert bool(((a / c["unit"]) == (a / c["unit"]).round()).all()) and bool((c["dY"] == c["dY"].round()).all()), row.id
            for s in we.blocks(row.N):
                assert bool((c["dY"][:, s] != 0).any(1).all()), (row.id, "a row of dY is zero in block", s)
            for s in we.blocks(row.K):
                assert bool((a[:, s] != 0).any(1).all()), (row.id, "a row of act(X) is zero in block", s)
            assert float(c["X"].abs().max()) < we.PAD_VALUE * 16 and float(c["dY"].abs().max()) < we.PAD_VALUE * 16
    print("largest sum of |products| of a split: %.0f units (limit 2^24 = %.0f)" % (worst, we.LIMIT))


# ---- what the older bound sees ----------------------------------------------------------------------------------------------------------------------
OLD_TOL = {"f32": 2e-4, "bf16": 3e-4}          # of the result's global maximum (tests/test_gpu_kernels.py, tests/test_gpu_bf16.py)


def _fault_rows():
    """one "tail1" row per template with scale / shift, ragged in K"""
    out = {}
    for row in wr.EXACT_TABLE:
        t = row.inst.template
        if t not in out and "tail1" in row.want and wr.VIEWS[row.view][1] and row.K % 32 and row.view != "hs3":
            out[t] = row
    assert sorted(out) == [0, 1, 2, 3]
    return out


def test_what_equality_sees_and_whether_the_old_bound_does():
    """Three faults modelled on the REFERENCE.  (a) the last row of the last split is dropped; (b) one chunk — the first of the second split — is counted
    twice; (c) the constants slip by one at the ragged edge.  Taken literally — scale / shift of channel K - 1 applied to padding channel K —
    that fault is INVISIBLE by construction: column K of dW is stored by no kernel (`ci < K`), so no test of dW, exact or not, can see it.  What is
    modelled is the same slip seen from the stored side: channel K - 1 is read through the padding channel's constants (scale 1, shift 0).
    Equality must see each; whether |fault - ref| <= tol * max|ref| (the older tests' bound, on these inputs) does is printed."""
    hidden = 0
    for t, row in sorted(_fault_rows().items()):
        r, g = wr.check_regime(row)
        c = we.case(row)
        want = we.ref(c)["dw"]
        sl = we.split_slices(g, row.M)
        faults = {"last row dropped": we.ref(c, slice(0, row.M - 1))["dw"],
                  "chunk counted twice": want + we.ref(c, slice(sl[1].start, sl[1].start + g.kc))["dw"]}
        c2 = dict(c, scale=c["scale"].clone(), shift=c["shift"].clone())
        c2["scale"][-1], c2["shift"][-1] = 1.0, 0.0
        faults["edge channel's constants slipped"] = we.ref(c2)["dw"]
        for what, got in faults.items():
            assert not torch.equal(we.f32(got), we.f32(want)), (row.id, what, "equality does not see the fault")
            err, top = float((got - want).abs().max()), float(want.abs().max())
            seen = err > OLD_TOL[row.inst.type] * top
            hidden += not seen
            print("%-34s %-36s |fault - ref| max %8.3f = %.2e of max|dW| %.1f: the %.0e bound %s" % (
                wr.inst_name(row.inst), what, err, err / top, top, OLD_TOL[row.inst.type], "SEES it" if seen else "does NOT see it"))
    print("%d of 12 modelled faults pass the relative-to-maximum bound; equality sees all 12" % hidden)


# ---- what the direct calls of the older tests reach -------------------------------------------------------------------------------------------------
def _old_direct_calls():
    """(bf16, M, K, N, act, view, bias) of every direct mny_pw_wgrad[_bf16] call of tests/test_gpu_kernels.py, test_gpu_fuzz.py and test_gpu_bf16.py:
    a TRANSCRIPTION of their shape lists and random sequences as they stood when tests/test_gpu_wgrad_exact.py was added.  It does not follow later
    edits of those files."""
    calls = []
    # test_gpu_kernels.py::test_pw_forward_wgrad_dgrad (view, bias gradient)
    for M, K, N, act in [(300, 32, 16, 0), (1000, 16, 96, 1), (777, 24, 144, 1), (513, 144, 24, 2), (242, 1280, 512, 1), (1024, 512, 512, 2), (484, 1024, 75, 2),
                         (130, 96, 576, 0), (257, 960, 160, 1), (64, 320, 1280, 0), (100, 512, 1024, 2)]:
        calls.append((0, M, K, N, act, True, True))
    # test_gpu_fuzz.py::test_pointwise_gemm_shapes
    r = np.random.RandomState(0)
    ks = [4, 8, 12, 16, 20, 24, 32, 36, 48, 64, 100, 160, 516]
    ns = [1, 3, 4, 10, 16, 31, 32, 33, 75, 96, 100, 128, 144, 160, 161, 320, 512]
    ms = [1, 5, 63, 64, 127, 128, 129, 255, 300, 1000, 4097]
    for trial in range(40):
        M, K, N = int(r.choice(ms)), int(r.choice(ks)), int(r.choice(ns))
        act = int(r.randint(0, 4))
        calls.append((0, M, K, N, act, True, True))
    # test_gpu_fuzz.py::test_barrier_free_matrix_core_kernel_shapes, form 1: a conv K -> N behind a view and its mirror image without, direct and deferred
    r = np.random.RandomState(11)
    for trial in range(24):
        K = 4 * int(r.randint(13, 25))
        N = int(r.choice([64, 96, 128, 192, 256, 288, 384, 512, 576]))
        if N < K:
            N = 192
        M = int(r.choice([8192, 8192 + 31, 8224, 16384, 16400, 20480 + 1, 4 * 128 * 32 * 2 + 32, int(r.randint(8192, 70000)), 16 * int(r.randint(1024, 4000))]))
        act = int(r.randint(0, 4))
        if trial % 4 == 1:
            calls += [(0, M, K, N, act, True, False), (0, M, N, K, 0, False, False)]
    # test_gpu_kernels.py: the 128 x 256 tile; the six-product accuracy test (and its special-values script); the route cases; the traffic script; the stream kernel
    calls += [(0, M, K, N, 1, True, False) for M, K, N in [(30976, 512, 512), (7757, 1280, 512), (20011, 256, 128)]]
    calls += [(0, M, K, N, 0, False, False) for M, K, N in [(4096, 512, 512), (4100, 96, 576), (3000, 960, 160), (5000, 64, 384), (2049, 1280, 512)]]
    calls += [(0, 500, 30, 36, 0, False, False), (0, 16384, 64, 384, 0, False, False), (1, 500, 36, 40, 0, False, False)]
    calls += [(0, M, K, N, 1, True, False) for M, K, N in [(123904, 64, 384), (30976, 512, 512), (123904, 96, 576), (123904, 512, 512), (30976, 160, 960)]]
    for M, K, N, act in [(16384, 96, 576, 1), (20480, 576, 96, 1), (16400, 64, 384, 2), (32768, 384, 64, 0), (16384, 96, 192, 4), (17008, 192, 64, 3),
                         (30976, 160, 960, 1), (16384, 576, 160, 1), (16384, 128, 256, 2), (16384, 960, 320, 1), (16384, 320, 1280, 2)]:
        calls += [(0, M, K, N, act, True, False), (0, M, K, N, 0, False, False)]
    # test_gpu_bf16.py::test_pw_bf16 (view, bias gradient)
    for M, K, N, act in [(300, 32, 16, 0), (1000, 16, 96, 1), (513, 144, 24, 2), (242, 1280, 512, 4), (484, 1024, 75, 2), (700, 10, 40, 3), (700, 40, 10, 0),
                         (257, 960, 160, 1), (333, 28, 112, 3), (5000, 72, 24, 4), (3001, 120, 40, 3), (4096, 128, 128, 2), (70, 672, 160, 4), (9000, 16, 64, 1),
                         (2500, 184, 80, 4), (131109, 16, 64, 3), (140000, 16, 16, 1), (131075, 24, 72, 4), (131072, 40, 120, 3), (131080, 40, 240, 4),
                         (131073, 48, 8, 2), (131072, 16, 96, 1), (131074, 40, 200, 4)]:
        calls.append((1, M, K, N, act, True, True))
    return calls


OLD_REACH = {"pw_wgrad_kernel<float>": 10, "pw_wgrad_kernel<bf16_t>": 5, "pw_wgrad_dma_kernel X6=0": 12, "pw_wgrad_dma_kernel X6=1": 4, "pw_wgrad_bf16_kernel": 14}


def test_what_the_direct_calls_of_the_older_tests_reach():
    """Counts the instantiations the older tests' direct calls launched when the exact tests were added (the whole-network tests launch more, at
    network-parity tolerances), prints them and pins the counts quoted in LAB_NOTES.md.  The shapes are a transcription (_old_direct_calls): the figure
    records that moment — a change of the PLAN moves it and fails here, a later edit of the older tests does not."""
    hit = {wr.route(*c).inst for c in _old_direct_calls()} - {None}
    assert hit <= set(wr.ROWS)

    def group(i):
        if i.template == wr.T_REG:
            return "pw_wgrad_kernel<%s>" % ("bf16_t" if i.type == "bf16" else "float")
        return "pw_wgrad_bf16_kernel" if i.template == wr.T_BF16 else "pw_wgrad_dma_kernel X6=%d" % i.variant
    got = {}
    for i in wr.ROWS:
        got.setdefault(group(i), [0, 0])
        got[group(i)][1] += 1
        got[group(i)][0] += i in hit
    for k, (a, b) in got.items():
        print("%-28s reached by the older direct calls: %2d of %2d; never: %s" % (k, a, b, " ".join(wr.inst_name(i).split("<")[1][:-1] for i in wr.ROWS if group(i) == k and i not in hit)))
    print("in all %d of %d; tests/wgrad_regimes.py TABLE: %d of %d" % (len(hit), len(wr.ROWS), len({wr.check_regime(r)[0].inst for r in wr.TABLE}), len(wr.ROWS)))
    assert not any(i.template == wr.T_BF16 and i.variant == 0 for i in hit), "(no bf16 LDS-DMA kernel had run without a view)"
    assert {k: v[0] for k, v in got.items()} == OLD_REACH, {k: v[0] for k, v in got.items()}
