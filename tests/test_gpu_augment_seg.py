"""Device-side seg maps (mny_aug_seg_batch through TrainAugment(seg_classes=...)) against the reference fixtures
(tools/gen_golden_augment_seg.py) and the numpy restatement (tests/augment_seg_ref.py): the same fp64 tap tables and the
same fp32 operations in the same order -> compared BIT FOR BIT."""
import glob
import json
import os
import random

import numpy as np
import pytest
import torch

import augment_ref as A
import augment_seg_ref as S

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
MEAN, STD = [0.5, 0.5, 0.5], [1, 1, 1]                           # models/bdd100k/config.yaml
SCALE = 1.3


@pytest.fixture(scope="module")
def M():
    assert torch.cuda.is_available()
    from mobilenet_yolo_pytorch_amd import augment
    return augment


def id_map(r, h, w, max_id):
    """Uniform regions with noisy patches; ids 0..max_id."""
    m = np.kron(r.randint(0, max_id + 1, size=(5, 4)), np.ones((h // 5 + 1, w // 4 + 1))).astype(np.uint8)[:h, :w]
    noise = r.randint(0, max_id + 1, size=(h, w)).astype(np.uint8)
    return np.where(r.rand(h, w) < 0.15, noise, m)


def random_groups(n, seed, max_id, lo=60, hi=300):
    from mobilenet_yolo_pytorch_amd import synthetic
    r = np.random.RandomState(seed)
    shapes = [(int(r.randint(lo, hi)), int(r.randint(lo, hi))) for _ in range(n)]
    photos = synthetic.photos(shapes, seed=seed)
    tg = [t.numpy() for t in synthetic.targets(n, seed=seed + 1, boxes_per_image=3, empty_every=4)]
    return [[(p, t, id_map(r, p.shape[0], p.shape[1], max_id))] for p, t in zip(photos, tg)]


def restated(groups, seed, sizes, C, size=None):
    """(maps, samples, size) of the restatement for TrainAugment(rng=Random(seed))(groups)."""
    samples, drawn, _ = A.plan(random.Random(seed), [[(im.shape[0], im.shape[1], t)] for (im, t, _), in groups], SCALE, 1000, sizes)
    size = size or drawn
    return S.batch_maps([g[0][2] for g in groups], [s["members"][0] for s in samples], C, size), samples, size


@pytest.mark.parametrize("name", sorted(os.path.basename(p) for p in glob.glob(os.path.join(G, "augseg_*.npz"))))
def test_reference_fixture_bit_exact(M, name):
    z = np.load(os.path.join(G, name))
    n, C = int(z["count"]), int(z["seg_classes"])
    groups = [[(z["img%d" % i], z["tgt%d" % i], z["seg%d" % i])] for i in range(n)]
    mk = lambda **kw: M.TrainAugment(z["sizes"].tolist(), MEAN, STD, float(z["expand_scale"]), rng=random.Random(int(z["seed"])), **kw)
    aug = mk(seg_classes=C)
    images, targets, count, maps = aug(groups)
    aug.check()
    size = tuple(int(v) for v in z["size"])
    grid = (size[0] // 16, size[1] // 16)
    assert count == n and maps.dtype == torch.float32 and tuple(maps.shape) == (n,) + grid + (C,) and maps.is_cuda
    got = maps.cpu().numpy()
    for i in range(n):
        assert np.array_equal(got[i], S.seg_maps(z["new_seg%d" % i], C, grid)), i          # the id map the REFERENCE handed to collate_fn
        assert np.array_equal(targets[i].numpy(), z["out_tgt%d" % i]), i
    plain = mk()(([[m[:2] for m in g] for g in groups]))
    assert len(plain) == 3 and torch.equal(plain[0], images)


@pytest.mark.parametrize("size,C,max_id", [(96, 2, 3), (160, 2, 3), (416, 2, 3), (160, 1, 2), (416, 8, 9)])
def test_random_batch_bit_exact(M, size, C, max_id):
    groups = random_groups(8, seed=size + C, max_id=max_id)
    sizes = [[size, size]]
    ref, samples, _ = restated(groups, 5, sizes, C)
    outs = []
    for _ in range(2):
        aug = M.TrainAugment(sizes, MEAN, STD, SCALE, rng=random.Random(5), seg_classes=C)
        images, targets, count, maps = aug(groups)
        aug.check()
        outs.append(maps.cpu().numpy())
    assert outs[0].shape == ref.shape == (8, size // 16, size // 16, C)
    assert np.array_equal(outs[0], ref)
    assert np.array_equal(outs[0], outs[1])                                                  # launch to launch
    assert all(np.array_equal(t.numpy(), s["target"].numpy()) for t, s in zip(targets, samples))
    assert all(np.count_nonzero((ref[..., c] > 0) & (ref[..., c] < 1)) for c in range(C))    # partial cells occur in every class
    plain = M.TrainAugment(sizes, MEAN, STD, SCALE, rng=random.Random(5))([[m[:2] for m in g] for g in groups])
    assert torch.equal(plain[0], images)                                                     # the image leg does not notice the seg leg


def run_cases(M, cases, C, size, out=None, damage=None):
    """cases: [(seg_id, expand or None, crop or None, flip)] -> (maps on the device, aug); one hand-made single-image plan each."""
    aug = M.TrainAugment([[size, size]], MEAN, STD, SCALE, seg_classes=C)
    items, samples = np.zeros(len(cases), M.ITEM), np.zeros(len(cases), M.SAMPLE)
    for k, (sg, exp, crop, flip) in enumerate(cases):
        h, w = sg.shape
        exp = exp or (h, w, 0, 0)
        items[k]["h"], items[k]["w"], items[k]["exp"], items[k]["crop"] = h, w, exp, crop or (0, 0, exp[0], exp[1])
        items[k]["flip"], items[k]["sample"] = int(flip), k
        samples[k] = (k, 1, -1, 0)
    if damage:
        damage(items, samples)
    plan = dict(items=items, samples=samples, size=(size, size), max_h=int(max(items["exp"][:, 0].max(), items["h"].max())),
                max_w=int(max(items["exp"][:, 1].max(), items["w"].max())))
    stage, offsets = aug.pack_seg([[(np.empty(sg.shape + (0,), np.uint8), None, sg)] for sg, _, _, _ in cases])
    return aug.run_device_seg(stage.to("cuda:0"), offsets, plan, out=out), aug


def geometry_cases(g, r, max_id):
    """Every path of the kernel at grid g: see the names."""
    a = lambda h, w: id_map(r, h, w, max_id)
    return {
        "identity": (a(61, 97), None, None, False),
        "flip_odd_width": (a(75, 91), None, None, True),
        "expand_border": (a(64, 80), (3 * 64, 3 * 80, 100, 130), None, False),          # whole grid cells lie in the border
        "expand_crop_flip": (a(70, 66), (90, 99, 13, 21), (5, 9, 71, 83), True),
        "crop_is_grid": (a(67, 83), None, (11, 17, g, g), True),                          # scale 1 on both axes
        "integer_scale": (a(52, 78), None, (0, 0, 2 * g, 3 * g), False),                  # ResizeAreaFast
        "integer_scale_flip": (a(4 * g + 5, 2 * g + 3), None, (3, 1, 4 * g, 2 * g), True),
        "one_axis_integer": (a(2 * g, 97), None, None, False),                            # general path all the same
        "tall_band": (a(1100, 60), None, None, True),                                     # at g=26, C=8: 43 rows > one 38-row LDS chunk
    }


@pytest.mark.parametrize("size,C,max_id", [(96, 2, 3), (160, 3, 3), (416, 8, 9)])
def test_geometry_cases_bit_exact(M, size, C, max_id):
    g = size // 16
    cases = geometry_cases(g, np.random.RandomState(size), max_id)
    got, aug = run_cases(M, list(cases.values()), C, size)
    aug.check()
    got = got.cpu().numpy()
    for k, (name, (sg, exp, crop, flip)) in enumerate(cases.items()):
        ref = S.seg_maps(S.geometry(sg, exp, crop, flip), C, (g, g))
        assert np.array_equal(got[k], ref), name
        assert ref.any(), name
    k = list(cases).index("expand_border")
    border = S.seg_maps(S.geometry(np.full((64, 80), 1, np.uint8), cases["expand_border"][1], None, False), 1, (g, g))[..., 0] == 0
    assert border.sum() >= g * g // 3 and np.all(got[k][border] == 0.0)                      # exact zeros in every class
    sg, _, crop, _ = cases["crop_is_grid"]
    win = sg[crop[0]:crop[0] + g, crop[1]:crop[1] + g][:, ::-1]
    assert np.array_equal(got[list(cases).index("crop_is_grid")], np.stack([(win == c).astype(np.float32) for c in range(1, C + 1)], -1))
    if size == 416:
        assert S.area_is_fast(52, 26) and S.area_is_fast(78, 26) and not S.area_is_fast(1100, 26)
        assert len(S.area_tab(1100, 26)[3]) > (8192 - 26 * C) // (26 * C)                   # the band really spans two chunks


def test_real_shape_bit_exact(M):
    """One 720x1280 id map -> 26x26 (scales 27.7 / 49.2), the BDD100K case."""
    sg = id_map(np.random.RandomState(7), 720, 1280, 3)
    got, aug = run_cases(M, [(sg, None, None, False)], 2, 416)
    aug.check()
    assert np.array_equal(got.cpu().numpy()[0], S.seg_maps(sg, 2, (26, 26)))


def test_bounds_flag_without_overrun(M):
    r = np.random.RandomState(3)
    cases = [(id_map(r, 70 + 9 * k, 90 + 5 * k, 3), None, None, bool(k & 1)) for k in range(5)]
    n, g, C = len(cases), 6, 2

    def too_small(items, samples):
        items["crop"][1] = (0, 0, g - 1, 40)                      # smaller than the grid: the scale < 1 path, must not be drawn

    guard = torch.full((n + 1, g, g, C), 7.0, device="cuda:0")
    out, aug = run_cases(M, cases, C, 96, out=guard[:n], damage=too_small)
    with pytest.raises(RuntimeError, match="seg map 1 "):
        aug.check()
    v = guard.cpu().numpy()
    assert np.all(v[n] == 7.0)                                    # nothing written past the batch
    assert np.all(v[1] == 0.0)                                    # the rejected sample is zero-filled
    for k in (0, 2, 3, 4):
        assert np.array_equal(v[k], S.seg_maps(S.geometry(*cases[k]), C, (g, g))), k

    def two_items(items, samples):
        samples["n_items"][3] = 2                                 # a mosaic record: not defined with seg maps

    guard.fill_(7.0)
    out, aug = run_cases(M, cases, C, 96, out=guard[:n], damage=two_items)
    with pytest.raises(RuntimeError, match="sample record 3 "):
        aug.check()
    v = guard.cpu().numpy()
    assert np.all(v[n] == 7.0) and np.all(v[3] == 0.0) and v[2].any()

    def huge(items, samples):
        items["h"][4] = 4000                                      # taller than its own canvas: must not be read

    guard.fill_(7.0)
    out, aug = run_cases(M, cases, C, 96, out=guard[:n], damage=huge)
    with pytest.raises(RuntimeError, match="seg map 4 "):
        aug.check()
    v = guard.cpu().numpy()
    assert np.all(v[n] == 7.0) and np.all(v[4] == 0.0) and v[0].any()
    out, aug = run_cases(M, cases, C, 96, out=guard[:n])
    aug.check()                                                   # the undamaged batch is clean


def test_argument_errors(M):
    from mobilenet_yolo_pytorch_amd._lib import MnyError
    sg = id_map(np.random.RandomState(1), 64, 64, 3)
    aug = M.TrainAugment([[96, 96]], MEAN, STD, SCALE, seg_classes=2)
    aug.seg_classes = 9                                           # past the constructor's check: the library refuses on the host
    plan = dict(items=np.zeros(1, M.ITEM), samples=np.zeros(1, M.SAMPLE), size=(96, 96), max_h=64, max_w=64)
    stage, offsets = aug.pack_seg([[(np.empty((64, 64, 0), np.uint8), None, sg)]])
    with pytest.raises(MnyError):
        aug.run_device_seg(stage.to("cuda:0"), offsets, plan)


def test_bdd_train_step_on_augmented_batch(M):
    """One training step of the BDD100K config on the device batch: finite losses, and the seg loss of the device maps equals
    the seg loss of the restatement's maps."""
    from mobilenet_yolo_pytorch_amd import yolo
    from oracle import procedural
    cfg = json.load(open(os.path.join(G, "state_keys_bdd100k.json")))["config"]
    cfg = dict(cfg, train_img_size=[[96, 96]])
    groups = random_groups(2, seed=31, max_id=3, lo=80, hi=200)
    aug = M.TrainAugment.from_config(cfg, rng=random.Random(4))
    assert aug.seg_classes == cfg["seg"]["num_classes"] == 2
    images, targets, count, maps = aug(groups)
    aug.check()
    ref, samples, _ = restated(groups, 4, [[96, 96]], 2)
    assert cfg["expand_scale"] == SCALE and np.array_equal(maps.cpu().numpy(), ref)
    torch.manual_seed(0)
    m = yolo(cfg, sync_metrics=True)
    procedural.fill_state_dict_(m)
    m = m.cuda().train()
    res, seg_out = m(images, [t.clone() for t in targets], maps)
    (sum(r[0] for r in res) + seg_out[0]).backward()
    vals = [float(r[0].detach()) for r in res] + [float(seg_out[0].detach())]
    assert all(np.isfinite(v) for v in vals) and vals[2] > 0
    res2, seg_ref = m(images, [s["target"].clone() for s in samples], torch.from_numpy(ref))
    assert vals[2] == float(seg_ref[0].detach()) and seg_out[1] == seg_ref[1] and seg_out[2] == seg_ref[2]
    assert [float(r[0].detach()) for r in res2] == vals[:2]
