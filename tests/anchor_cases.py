"""The inputs of the anchor-fitting tests, in one place: tests/test_anchor_ref_cpu.py asserts on the CPU that every k-means input
converges in the restatement (tests/anchor_ref.py) within MAX_STEPS, tests/test_gpu_anchors.py runs the same inputs through
csrc/anchors.hip.  Inputs are regenerated from the seed; nothing is stored.  Sizes: N = 1, 63, 64, 65 (one wave and its neighbours),
257 (a second tile slot of lane 0), 70 001 (69 workgroups, the last one partial) and 600 001 (more tiles than workgroups: the
grid-stride loop); k = 1, 6, 9, 32."""
import functools

import numpy as np

import anchor_ref as R

F32 = np.float32
MAX_STEPS = 200


def _integer(n, seed, lo=4, hi=400):
    return np.random.default_rng(seed).integers(lo, hi, (n, 2)).astype(F32)


def _uniform(n, seed):
    return np.random.default_rng(seed).uniform(6.0, 330.0, (n, 2)).astype(F32)


def _lognormal(n, seed):
    r = np.random.default_rng(seed)
    area = np.exp(r.normal(8.3, 1.2, n))
    ratio = np.exp(r.normal(0.0, 0.45, n))
    return np.clip(np.stack((np.sqrt(area * ratio), np.sqrt(area / ratio)), 1), 2.0, 640.0).astype(F32)


def _invalid(n, seed):
    wh = _uniform(n, seed)
    bad = [(0.0, 10.0), (10.0, 0.0), (-5.0, 20.0), (np.nan, 30.0), (30.0, np.nan), (np.inf, 40.0), (1e6, 50.0), (50.0, 70000.0), (2.0 ** -21, 8.0)]
    for i, b in enumerate(bad):
        wh[(7 * i + 3) % n] = b
    wh[n - 1] = (np.nan, np.nan)
    wh[0] = (2.0 ** -20, 65536.0)                      # both limits are valid
    return wh


# name: (maker, N, seed, k, explicit init or None)
KMEANS = {
    "n1-k1": (_integer, 1, 0, 1, None),
    "n37-k6": (_uniform, 37, 1, 6, None),
    "n63-k6": (_integer, 63, 2, 6, None),
    "n64-k9": (_uniform, 64, 3, 9, None),
    "n65-k32": (_lognormal, 65, 4, 32, None),
    "n257-k9": (_lognormal, 257, 5, 9, None),
    "int-1000-k6": (_integer, 1000, 6, 6, None),
    "uniform-5000-k6": (_uniform, 5000, 7, 6, None),
    "lognormal-70001-k9": (_lognormal, 70001, 8, 9, None),
    "invalid-300-k6": (_invalid, 300, 9, 6, None),
    # the last centre is smaller than every box by so much that it is nobody's best: it keeps its value through every step
    "empty-cluster-257-k3": (_uniform, 257, 10, 3, [(40.0, 40.0), (200.0, 200.0), (0.5, 0.25)]),
    # every IoU ties: all boxes go to centre 0, the other centres stay empty
    "identical-257-k6": (lambda n, seed: np.tile(np.array([[37.0, 91.0]], F32), (n, 1)), 257, 0, 6, None),
}


@functools.lru_cache(maxsize=None)
def kmeans_case(name):
    """-> (wh [N,2] fp32, k, init [k,2] fp32)"""
    maker, n, seed, k, init = KMEANS[name]
    wh = maker(n, seed)
    init = R.default_init(wh, k) if init is None else np.array(init, F32)
    wh.setflags(write=False)
    init.setflags(write=False)
    return wh, k, init


@functools.lru_cache(maxsize=None)
def kmeans_ref(name):
    """The restatement's run of a case, computed once and shared."""
    wh, k, init = kmeans_case(name)
    return R.kmeans(wh, init, MAX_STEPS, trace=True)


def candidates(wh, P, k, seed):
    """P candidate sets around the quantile init; set 0 is the init itself."""
    base = R.default_init(wh, k)
    f = np.random.default_rng(seed).uniform(0.6, 1.6, (P, k, 2)).astype(F32)
    f[0] = 1
    return (base[None] * f).astype(F32)


# name: (maker, N, seed, P, k)
FITNESS = {
    "n1-p1-k1": (_integer, 1, 20, 1, 1),
    "n63-p8-k6": (_uniform, 63, 21, 8, 6),
    "n64-p8-k9": (_integer, 64, 22, 8, 9),
    "n65-p256-k6": (_lognormal, 65, 23, 256, 6),
    "n257-p256-k32": (_lognormal, 257, 24, 256, 32),       # 8 LDS stages of 32 candidate sets
    "n257-p8-k32-invalid": (_invalid, 257, 25, 8, 32),
    "n70001-p8-k9": (_lognormal, 70001, 26, 8, 9),
    "n600001-p1-k6": (_uniform, 600001, 27, 1, 6),
}

# name: (maker, N, seed, P, k); G = 20 generations each
G = 20
EVOLVE = {
    "n65-p8-k6": (_uniform, 65, 30, 8, 6),
    "n257-p256-k9": (_lognormal, 257, 31, 256, 9),
    "n257-p1-k6": (_integer, 257, 32, 1, 6),               # the parent alone: nothing can change
    "n300-p8-k6-invalid": (_invalid, 300, 33, 8, 6),
    "n70001-p8-k9": (_lognormal, 70001, 34, 8, 9),
}


def draw_factors(seed, G, P, k, mutation_prob=0.9, sigma=0.1):
    """anchors.draw_factors, restated (the draw is not part of the ABI; the GPU tests hand these to both sides)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    mask = rng.random((G, P, k, 2)) < mutation_prob
    scale = rng.random((G, P, 1, 1))
    normal = rng.standard_normal((G, P, k, 2))
    return np.clip(1.0 + mask * scale * normal * sigma, 0.3, 3.0).astype(F32)
