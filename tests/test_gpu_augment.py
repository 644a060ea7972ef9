"""Device-side training augmentation (mny_aug_photometric / mny_aug_batch through TrainAugment) against the reference
fixtures (tools/gen_golden_augment.py) and the numpy restatement (tests/augment_ref.py, pinned to Pillow): all integer
work plus the same fp32 divisions as torch -> compared BIT FOR BIT."""
import ctypes
import glob
import os
import random

import numpy as np
import pytest
import torch

import augment_ref as A

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
VOC_SIZES = [[352, 352], [320, 320], [288, 288], [384, 384], [416, 416]]       # models/voc/config.yaml train_img_size
VOC_MEAN, VOC_STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


@pytest.fixture(scope="module")
def M():
    assert torch.cuda.is_available()
    from mobilenet_yolo_pytorch_amd import augment
    return augment


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def photometric_dev(M, images, chains):
    """mny_aug_photometric on a list of uint8 images, one chain each."""
    from mobilenet_yolo_pytorch_amd._lib import call, query
    dev = torch.device("cuda:0")
    items = np.zeros(len(images), M.ITEM)
    offs, off = [], 0
    for im in images:
        offs.append(off)
        off += (im.size + 15) // 16 * 16
    buf = np.zeros(off, np.uint8)
    for it, im, chain, o in zip(items, images, chains, offs):
        buf[o:o + im.size] = im.reshape(-1)
        it["offset"], it["h"], it["w"], it["n_ops"] = o, im.shape[0], im.shape[1], len(chain)
        for k, (op, f) in enumerate(chain):
            it["op"][k] = op
            if op == M.HUE:
                it["hue_shift"] = M.hue_shift_u8(f)
            elif op == M.GAMMA:
                it["gamma_map"] = M.gamma_map(f)
            else:
                it["factor"][k] = f
    mh, mw = max(im.shape[0] for im in images), max(im.shape[1] for im in images)
    src = torch.from_numpy(buf).to(dev)
    dst = torch.zeros_like(src)
    it_dev = torch.from_numpy(items.view(np.uint8).copy()).to(dev)
    ws = torch.empty(query("mny_aug_ws_bytes", len(images), 0, 0, mh, mw, 0, 1, 1), device=dev, dtype=torch.uint8)
    call("mny_aug_photometric", _p(src), _p(it_dev), len(images), mh, mw, _p(dst), _p(ws), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    out = dst.cpu().numpy()
    assert int(ws[:4].view(torch.int32).item()) == 0
    return [out[o:o + im.size].reshape(im.shape) for o, im in zip(offs, images)]


@pytest.fixture(scope="module")
def cube():
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)


@pytest.mark.parametrize("op,fs", [(A.BRIGHTNESS, [0.5, 0.8137, 1.0, 1.2549, 1.5]), (A.CONTRAST, [0.5, 0.9, 1.33]),
                                   (A.SATURATION, [0.5, 0.77, 1.0, 1.41]), (A.HUE, [-18 / 255., -5.3 / 255., 0.0, 0.031, 17.99 / 255.]),
                                   (A.GAMMA, [0.55, 1.0, 1.45])])
def test_photometric_single_op_rgb_cube(M, cube, op, fs):
    for f in fs:
        got = photometric_dev(M, [cube], [[(op, f)]])[0]
        assert np.array_equal(got, A.OPS[op](cube, f)), (A.OP_NAMES[op], f)


def test_photometric_random_chains_on_photos(M):
    from mobilenet_yolo_pytorch_amd import synthetic
    r = random.Random(5)
    sizes = [(r.randint(20, 300), r.randint(20, 300)) for _ in range(40)]
    imgs = synthetic.photos(sizes, seed=9)
    chains = []
    for i in range(len(imgs)):
        order = list(range(5))
        r.shuffle(order)
        if i % 3 == 0:                                  # contrast after other ops
            order.remove(A.CONTRAST)
            order.append(A.CONTRAST)
        chains.append([(op, r.uniform(-18 / 255., 18 / 255.) if op == A.HUE else r.uniform(0.5, 1.5)) for op in order[:r.randint(0, 5)]])
    chains[1] = [(A.BRIGHTNESS, 1.4), (A.HUE, -0.05), (A.CONTRAST, 0.6), (A.SATURATION, 1.3), (A.GAMMA, 0.7)]
    got = photometric_dev(M, imgs, chains)
    for g, im, ch in zip(got, imgs, chains):
        assert np.array_equal(g, A.photometric(im, ch)), ch


def _load(name):
    z = np.load(os.path.join(G, name))
    n = int(z["count"])
    imgs = [z["img%d" % i] for i in range(n)]
    groups, k = [], 0
    for s in z["groups"]:
        groups.append([(imgs[k + j], z["tgt%d" % (k + j)]) for j in range(int(s))])
        k += int(s)
    return z, groups


@pytest.mark.parametrize("name", sorted(os.path.basename(p) for p in glob.glob(os.path.join(G, "aug_*.npz"))))
def test_reference_fixture_bit_exact(M, name):
    z, groups = _load(name)
    kw = dict(canvas=int(z["canvas"]), rng=random.Random(int(z["seed"])))
    aug = M.TrainAugment(z["sizes"].tolist(), z["mean"], z["std"], float(z["expand_scale"]), **kw)
    images, targets, count = aug(groups)
    aug.check()
    assert count == int(z["count"])
    assert images.shape == z["batch"].shape and np.array_equal(images.cpu().numpy(), z["batch"])
    for i, t in enumerate(targets):
        assert np.array_equal(t.numpy(), z["out_tgt%d" % i])
    # the uint8 stage: mean 0, std 1/255 gives the resized uint8 values exactly
    kw["rng"] = random.Random(int(z["seed"]))
    raw = M.TrainAugment(z["sizes"].tolist(), [0, 0, 0], [1 / 255.] * 3, float(z["expand_scale"]), **kw)(groups)[0].cpu().numpy()
    from oracle import prep_ref
    size = tuple(int(v) for v in z["size"])
    for i in range(len(groups)):
        assert np.array_equal(np.rint(raw[i]).astype(np.uint8).transpose(1, 2, 0), prep_ref.resize_bilinear_u8(z["u8_%d" % i], *size))


def voc_groups(n=256, seed=0):
    """VOC-shaped photos (500x375 and 375x500) under the reference's mix: 25 % 4-mosaics, the rest single."""
    from mobilenet_yolo_pytorch_amd import synthetic
    r = random.Random(seed)
    kinds = [4 if r.random() < 0.25 else 1 for _ in range(n)]
    shapes = [(375, 500) if r.random() < 0.7 else (500, 375) for _ in range(sum(kinds))]
    photos = synthetic.photos(shapes, seed=seed)
    tg = [t.numpy() for t in synthetic.targets(len(photos), seed=seed + 1, empty_every=7)]
    groups, k = [], 0
    for s in kinds:
        groups.append([(photos[k + j], tg[k + j]) for j in range(s)])
        k += s
    return groups


@pytest.fixture(scope="module")
def voc():
    groups = voc_groups()
    samples, _, _ = A.plan(random.Random(3), [[(im.shape[0], im.shape[1], t) for im, t in g] for g in groups], 2.1610954191879452, 1000, VOC_SIZES)
    u8 = [A.render_u8([im for im, _ in g], s, 1000) for g, s in zip(groups, samples)]
    return groups, samples, u8


@pytest.mark.parametrize("size", [tuple(s) for s in VOC_SIZES])
def test_voc_mix_batch_bit_exact(M, voc, size):
    groups, samples, u8 = voc
    aug = M.TrainAugment(VOC_SIZES, VOC_MEAN, VOC_STD, 2.1610954191879452, rng=random.Random(3))
    images, targets, count = aug(groups, size=size)
    aug.check()
    assert count == sum(len(g) for g in groups)
    got = images.cpu().numpy()
    for i in range(len(groups)):
        ref = A.collate([u8[i]], size, VOC_MEAN, VOC_STD)[0]
        assert np.array_equal(got[i], ref), i
        assert np.array_equal(targets[i].numpy(), samples[i]["target"].numpy()), i


def test_launch_to_launch_bit_equal(M):
    groups = voc_groups(48, seed=4)
    outs = []
    for _ in range(3):
        aug = M.TrainAugment(VOC_SIZES, VOC_MEAN, VOC_STD, 2.1610954191879452, rng=random.Random(8))
        outs.append(aug(groups)[0].cpu().numpy())
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


def test_bounds_flag_without_overrun(M):
    groups = voc_groups(6, seed=6)
    aug = M.TrainAugment([[64, 64]], VOC_MEAN, VOC_STD, 1.5, canvas=200, rng=random.Random(1))
    plan = aug.plan(groups)
    stage, offsets = aug.pack(groups)
    plan["items"]["offset"] = offsets
    bad = 0
    plan["items"]["h"][bad] = plan["max_h"] + 7                    # declared larger than the maximum: must not be read
    n = len(plan["samples"])
    guard = torch.full((n + 1, 3, 64, 64), 7.0, device="cuda:0")
    out = aug.run_device(stage.to("cuda:0"), plan, out=guard[:n])
    with pytest.raises(RuntimeError, match="image %d" % bad):
        aug.check()
    g = guard.cpu().numpy()
    assert np.all(g[n] == 7.0)                                      # nothing written past the batch
    assert np.all(g[int(plan["items"]["sample"][bad])] == 0.0)      # the rejected sample is zero-filled
    assert out.shape[0] == n and np.all(np.isfinite(g[:n]))
    assert any(np.any(g[i] != 0) for i in range(n) if i != int(plan["items"]["sample"][bad]))


def test_model_on_augmented_batch(M):
    """model(images, targets) on the device batch equals the same call on the restatement's batch."""
    from mobilenet_yolo_pytorch_amd import yolo
    from oracle import net_ref, procedural
    groups = voc_groups(4, seed=11)
    aug = M.TrainAugment([[96, 96]], VOC_MEAN, VOC_STD, 2.1610954191879452, rng=random.Random(2))
    images, targets, _ = aug(groups)
    samples, size, _ = A.plan(random.Random(2), [[(im.shape[0], im.shape[1], t) for im, t in g] for g in groups], 2.1610954191879452, 1000, [[96, 96]])
    ref = torch.from_numpy(A.collate([A.render_u8([im for im, _ in g], s, 1000) for g, s in zip(groups, samples)], size, VOC_MEAN, VOC_STD))
    torch.manual_seed(0)
    m = yolo(procedural.VOC_CONFIG, sync_metrics=True)
    m.load_state_dict(procedural.fill_state_dict_(net_ref.RefYolo(procedural.VOC_CONFIG)).state_dict())
    m = m.to("cuda:0").train()
    a = m(images, [t.clone() for t in targets])
    b = m(ref.to("cuda:0"), [s["target"].clone() for s in samples])
    for i in range(2):
        assert float(a[i][0]) == float(b[i][0])
