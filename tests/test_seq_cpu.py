"""CPU: the host half of the blur / sharpen / noise stage (augment.SeqAugment: draws, records) and the sanity of its restatement
(tests/seq_ref.py).  No GPU and no library call."""
import math
import random
import re
import os

import numpy as np
import pytest

import seq_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 20000


@pytest.fixture(scope="module")
def M():
    from mobilenet_yolo_pytorch_amd import augment
    return augment


@pytest.fixture(scope="module")
def drawn(M):
    s = M.SeqAugment(seed=11)
    d = s.draw(N)
    return d, M.SeqAugment.records(d)


def within(k, n, p):
    """k successes of n at probability p lie within 5 binomial standard deviations."""
    return abs(k - n * p) <= 5 * math.sqrt(n * p * (1 - p))


def test_plan_is_a_function_of_the_seed(M):
    a, b, c = M.SeqAugment(seed=5).plan(300), M.SeqAugment(seed=5).plan(300), M.SeqAugment(seed=6).plan(300)
    assert a.dtype == M.SEQ and a.tobytes() == b.tobytes() and a.tobytes() != c.tobytes()
    s = M.SeqAugment(seed=5)
    first, second = s.plan(300), s.plan(300)                         # the generator advances from batch to batch
    assert first.tobytes() == a.tobytes() and second.tobytes() != a.tobytes()


def test_plan_never_touches_python_random(M):
    random.seed(1234)
    state = random.getstate()
    M.SeqAugment(seed=1).plan(500)
    M.SeqAugment().plan(10)
    assert random.getstate() == state


def test_train_augment_plan_does_not_notice_seq(M):
    from mobilenet_yolo_pytorch_amd import synthetic
    shapes = [(60, 67), (48, 50), (64, 40), (33, 61), (50, 50), (64, 64), (41, 57)]
    tg = [t.numpy() for t in synthetic.targets(len(shapes), seed=3, boxes_per_image=2)]
    groups = [[(shapes[0], tg[0])], [(shapes[1], tg[1])], [(s, t) for s, t in zip(shapes[2:6], tg[2:6])], [(shapes[6], tg[6])]]
    outs = []
    for seq in (None, M.SeqAugment(seed=2, device="cpu")):
        rng = random.Random(9)
        aug = M.TrainAugment([[32, 32], [64, 64]], [0.5] * 3, [1.0] * 3, 1.5, device="cpu", rng=rng, seq=seq)
        p = aug.plan(groups)
        outs.append((p, rng.getstate()))
    (p0, s0), (p1, s1) = outs
    assert s0 == s1 and p0["items"].tobytes() == p1["items"].tobytes() and p0["samples"].tobytes() == p1["samples"].tobytes()
    assert p0["count"] == p1["count"] == 7 and p0["size"] == p1["size"]
    assert all(np.array_equal(a.numpy(), b.numpy()) for a, b in zip(p0["targets"], p1["targets"]))


def test_draw_frequencies(drawn):
    d, _ = drawn
    gate = d["gate"]
    g = int(gate.sum())
    assert within(g, N, 0.5)
    assert within(int((d["count"][gate] == 1).sum()), g, 0.5)
    chosen = np.zeros((N, 3), bool)
    for i in range(N):
        chosen[i, d["order"][i][:d["count"][i]]] = True
    for child in range(3):
        assert within(int(chosen[gate, child].sum()), g, 0.5), child
    assert all(sorted(o) == [0, 1, 2] for o in d["order"][:200])
    blur = gate & chosen[:, 0]
    assert within(int(d["gauss"][blur].sum()), int(blur.sum()), 0.5)
    med = blur & ~d["gauss"]
    assert set(np.unique(d["k"])) == {3, 5}
    assert within(int((d["k"][med] == 3).sum()), int(med.sum()), 1 / 3)
    noisy = gate & chosen[:, 2]
    assert within(int(d["per_channel"][noisy].sum()), int(noisy.sum()), 0.3)


def test_parameter_ranges(drawn):
    d, _ = drawn
    for name, lo, hi in (("sigma", 0.0, 1.0), ("alpha", 0.0, 0.1), ("lightness", 0.9, 1.1), ("scale", 0.0, 0.03 * 255)):
        assert d[name].min() >= lo and d[name].max() <= hi, name
        assert d[name].max() - d[name].min() > 0.95 * (hi - lo), name            # and the range is used
    assert len(np.unique(d["key"])) == N and int(d["key"].max()) > 2 ** 63


def test_records_follow_the_draws(M, drawn):
    d, rec = drawn
    kinds = {M.SEQ_GAUSS, M.SEQ_MEDIAN, M.SEQ_SHARPEN, M.SEQ_NOISE}
    assert len(kinds) == 4 and (M.SEQ_GAUSS, M.SEQ_MEDIAN, M.SEQ_SHARPEN, M.SEQ_NOISE) == (R.GAUSS, R.MEDIAN, R.SHARPEN, R.NOISE)
    assert np.all(rec["n_ops"][~d["gate"]] == 0)
    tiny = d["sigma"] < 1e-3
    for i in range(N):
        r = rec[i]
        ops = [int(o) for o in r["op"][:r["n_ops"]]]
        assert len(set(ops)) == len(ops) and set(ops) <= kinds                          # no kind twice
        if not d["gate"][i]:
            continue
        want = []
        for child in d["order"][i][:d["count"][i]]:
            if child == 0:
                if d["gauss"][i]:
                    if not tiny[i]:
                        want.append(M.SEQ_GAUSS)
                else:
                    want.append(M.SEQ_MEDIAN)
            else:
                want.append(M.SEQ_SHARPEN if child == 1 else M.SEQ_NOISE)
        assert ops == want, i
        if M.SEQ_MEDIAN in ops:
            assert r["median_k"] == d["k"][i]
        if M.SEQ_GAUSS in ops:
            assert np.array_equal(r["taps"], R.taps(d["sigma"][i]))
        if M.SEQ_SHARPEN in ops:
            assert (r["sharpen_c"], r["sharpen_s"]) == R.sharpen_coeffs(d["alpha"][i], d["lightness"][i])
        if M.SEQ_NOISE in ops:
            assert r["noise_scale"] == np.float32(d["scale"][i]) and r["noise_per_channel"] == int(d["per_channel"][i])
            assert int(r["noise_key"][0]) | (int(r["noise_key"][1]) << 32) == int(d["key"][i])
    assert np.isfinite(rec["taps"]).all() and np.isfinite(rec["sharpen_c"]).all()


def test_tiny_sigma_emits_no_op(M):
    rec = M.seq_records([[(M.SEQ_GAUSS, 5e-4)], [(M.SEQ_GAUSS, 5e-4), (M.SEQ_NOISE, 1.0, False, 7)], [(M.SEQ_GAUSS, 2e-3)]])
    assert rec["n_ops"].tolist() == [0, 1, 1] and rec["op"][1][0] == M.SEQ_NOISE and rec["op"][2][0] == M.SEQ_GAUSS
    with pytest.raises(ValueError):
        M.seq_records([[(M.SEQ_SHARPEN, 0.1, 1.0), (M.SEQ_SHARPEN, 0.05, 1.0)]])
    with pytest.raises(ValueError):
        M.seq_records([[(M.SEQ_MEDIAN, 4)]])
    fixed = M.SeqAugment.fixed([[(M.SEQ_MEDIAN, 5)], []], device="cpu")
    assert fixed.plan(2)["n_ops"].tolist() == [1, 0]
    with pytest.raises(ValueError):
        fixed.plan(3)


def test_struct_size_matches_the_header(M):
    src = open(os.path.join(REPO, "include", "mnyolo.h")).read()
    m = re.search(r"\}\s*mny_aug_seq_item;\s*/\*\s*(\d+) bytes\s*\*/", src)
    assert m and int(m.group(1)) == M.SEQ.itemsize == 64
    body = src[src.index("typedef struct mny_aug_seq_item"):m.start()]
    fields = re.findall(r"\b(?:int32_t|uint32_t|float)\s+([^;]+);", body)
    names = [re.sub(r"\[\d+\]", "", n).strip() for f in fields for n in f.split(",")]
    assert names == list(M.SEQ.names)


# ---- the restatement itself ---------------------------------------------------------------------------------------
def test_philox_known_answers():
    """Random123's known answer for philox4x32-10 at counter 0, key 0."""
    assert [int(x) for x in R.philox4x32_10(np.array(0, np.uint64), (0, 0))] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]


def test_taps_and_fixed_points():
    for sigma in (0.05, 0.3, 0.5, 1.0):
        t = R.taps(sigma)
        assert t.dtype == np.float32 and abs(float(t.astype(np.float64).sum()) - 1) < 2e-7 and np.array_equal(t, t[::-1])
    assert R.taps(0.05).tolist() == [0, 0, 1, 0, 0]
    for h, w in ((1, 1), (2, 2), (1, 7), (9, 11)):
        for value in (0, 37, 255):
            a = np.full((h, w, 3), value, np.uint8)
            assert np.array_equal(R.gaussian(a, R.taps(0.8))[0], a)
            assert np.array_equal(R.median(a, 3)[0], a) and np.array_equal(R.median(a, 5)[0], a)
            assert np.array_equal(R.sharpen(a, *R.sharpen_coeffs(0.0, 1.0))[0], a)
    a = np.full((9, 11, 3), 37, np.uint8)                               # lightness 1: the kernel sums to one
    assert np.array_equal(R.sharpen(a, *R.sharpen_coeffs(0.1, 1.0))[0], a)
    r = np.random.RandomState(0).randint(0, 256, size=(6, 7, 3)).astype(np.uint8)
    assert np.array_equal(R.sharpen(r, *R.sharpen_coeffs(0.0, 1.1))[0], r)
    assert np.array_equal(R.noise(r, 0.0, True, (1, 2))[0], r)


def test_borders_by_hand():
    """REFLECT_101 and REPLICATE written out, down to sides of 1 and 2."""
    def reflect(i, n):
        if n == 1:
            return 0
        while i < 0 or i >= n:
            i = -i if i < 0 else 2 * (n - 1) - i
        return i
    r = np.random.RandomState(1)
    for h, w in ((1, 1), (1, 7), (2, 2), (3, 5), (6, 4)):
        a = r.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        t = R.taps(1.0).astype(np.float64)
        hp = np.zeros((h, w, 3))
        for y in range(h):
            for x in range(w):
                hp[y, x] = sum(t[d + 2] * a[y, reflect(x + d, w)] for d in range(-2, 3))
        want = np.zeros((h, w, 3))
        med = np.zeros((h, w, 3), np.uint8)
        for y in range(h):
            for x in range(w):
                want[y, x] = sum(t[d + 2] * hp[reflect(y + d, h), x] for d in range(-2, 3))
                win = [a[min(max(y + dy, 0), h - 1), min(max(x + dx, 0), w - 1)] for dy in range(-2, 3) for dx in range(-2, 3)]
                med[y, x] = np.sort(np.array(win), axis=0)[12]
        assert np.allclose(R.gaussian(a, R.taps(1.0))[1], want, atol=1e-9)
        assert np.array_equal(R.median(a, 5)[0], med)


def test_noise_stream_statistics():
    n = 1 << 20
    z = R.normals(np.arange(n, dtype=np.uint64), (0xdeadbeef, 0x12345678))
    for c in range(3):
        assert abs(z[c].mean()) < 5 / math.sqrt(n)
        assert abs(z[c].var() - 1) < 5 * math.sqrt(2 / n)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert abs(np.corrcoef(z[a], z[b])[0, 1]) < 5 / math.sqrt(n)
    img = np.full((64, 64, 3), 128, np.uint8)
    shared = R.noise(img, 7.65, False, (3, 4))[0].astype(int) - 128
    per = R.noise(img, 7.65, True, (3, 4))[0].astype(int) - 128
    assert np.array_equal(shared[..., 0], shared[..., 1]) and np.array_equal(shared[..., 0], shared[..., 2]) and shared.any()
    assert np.array_equal(per[..., 0], shared[..., 0]) and not np.array_equal(per[..., 0], per[..., 1])
    assert not np.array_equal(R.noise(img, 7.65, False, (3, 5))[0], R.noise(img, 7.65, False, (3, 4))[0])


def test_device_test_inputs_meet_the_band_precondition():
    """The rounded comparisons of tests/test_gpu_augment_seq.py allow a difference of one only within 1e-3 of a tie, and only if such
    values are rare: at most 2 % of the pixels of the larger images and one pixel of an image under 100 pixels.  That is a property of
    the inputs, settled here on the restatement alone."""
    ims = [a for _, _, a in R.images(0)]
    for sigma in R.GAUSS_SIGMAS:
        assert R.band_ok([R.gaussian(a, R.taps(sigma))[1] for a in ims]), sigma
    for alpha, l in R.SHARPEN_PARAMS:
        assert R.band_ok([R.sharpen(a, *R.sharpen_coeffs(alpha, l))[1] for a in ims]), (alpha, l)
    for scale in R.NOISE_SCALES:
        for per in (False, True):
            assert R.band_ok([R.noise(a, scale, per, R.noise_key(i))[1] for i, a in enumerate(ims)]), (scale, per)
