"""CPU: host-side logic of the stages around the path (no kernels run here) — input-prep packing, mAP list packing and
bookkeeping, the reference-shaped return contracts, and the loud failure without a GPU."""
import json
import os

import numpy as np
import pytest
import torch

G = os.path.join(os.path.dirname(__file__), "golden")


def test_batchprep_pack_layout_and_validation():
    from mobilenet_yolo_pytorch_amd import prep, synthetic
    bp = prep.BatchPrep([[352, 352], [320, 320]], [0.485, 0.456, 0.406], [0.229, 0.224, 0.225], device="cpu")
    imgs = synthetic.photos([(5, 7), (4, 4), (9, 3)], seed=1)
    stage, desc, mh, mw = bp.pack(imgs)
    assert (mh, mw) == (9, 7) and desc.dtype.itemsize == 16                       # mny_image_desc: int64 + 2 x int32
    assert all(int(o) % 16 == 0 for o in desc["offset"]) and list(desc["h"]) == [5, 4, 9] and list(desc["w"]) == [7, 4, 3]
    buf = stage.numpy()
    for d, im in zip(desc, imgs):
        assert np.array_equal(buf[d["offset"]:d["offset"] + im.size].reshape(im.shape), im)
    assert tuple(bp.choose_size()) in ((352, 352), (320, 320))
    with pytest.raises(ValueError):
        bp.pack([np.zeros((4, 4, 3), np.float32)])
    with pytest.raises(ValueError):
        bp([])


def test_map_list_packing_and_cpu_rejection():
    from mobilenet_yolo_pytorch_amd import evalmap
    ts = [torch.zeros(2, 4), torch.zeros(0, 4), torch.ones(3, 4)]
    flat, off = evalmap._pack_list(ts, 4, torch.device("cpu"))
    assert flat.shape == (5, 4) and off.tolist() == [0, 2, 2, 5] and off.dtype == torch.int32
    flat, off = evalmap._pack_list([torch.zeros(0), torch.ones(2)], 0, torch.device("cpu"))
    assert flat.shape == (2,) and off.tolist() == [0, 0, 2]
    z = torch.zeros(0)
    with pytest.raises(RuntimeError, match="CUDA"):
        evalmap.map_eval(torch.zeros(0, 4), z, z, torch.zeros(1, dtype=torch.int32), torch.zeros(0, 4), z, z, torch.zeros(1, dtype=torch.int32), 3)
    assert evalmap.adjust_confidence(10, 31, 0.1) == pytest.approx(0.11) and evalmap.adjust_confidence(10, 5, 0.01) == 0.01


def test_evaluator_bookkeeping():
    from mobilenet_yolo_pytorch_amd import evalmap
    ev = evalmap.Evaluator(["background", "a", "b"])
    ev.add([torch.zeros(3, 7), None], [torch.zeros(2, 5), np.zeros((0, 5), np.float32)])
    ev.add_packed(torch.zeros(4, 7), [1, 3], [torch.zeros(1, 5), torch.zeros(2, 5)])
    assert ev.row_counts == [3, 0, 1, 3] and ev.tg_counts == [2, 0, 1, 2] and ev.gt_box == 5 and ev.pred_box == 7


def test_seg_config_contract_without_gpu():
    from mobilenet_yolo_pytorch_amd import yolo
    man = json.load(open(os.path.join(G, "state_keys_bdd100k.json")))
    m = yolo(man["config"])
    assert m.has_seg and m.seg_num_classes == 2 and m.graph.seg_out is not None
    assert not yolo(json.load(open(os.path.join(G, "state_keys_voc.json")))["config"]).has_seg
    with pytest.raises(Exception):                 # CPU tensors: the HIP path is the only path
        m.train()(torch.zeros(1, 3, 96, 96), [torch.zeros(0, 5)], torch.zeros(1, 6, 6, 2))


@pytest.mark.timeout(180)
def test_bench_launches_its_own_ranks_for_gpus_gt_1_and_relays_one_json_line():
    """the driver starts `python bench.py --gpus N` for N = 1 and may do the same for N > 1.  Without a launcher's
    environment bench.py must start the N ranks itself as child processes (torch.distributed.run, 127.0.0.1 rendezvous) and hand
    rank 0's single JSON line and the exit code through.  --launch-check runs exactly that path with the ranks meeting over gloo
    on the CPU instead of running the GPU step."""
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--gpus", "2", "--launch-check"], capture_output=True, text=True, env=env, timeout=170)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    # parent_clean: the launcher parent had imported neither torch nor amdsmi nor this package when it started its ranks (VERDICT r3 #1:
    # on this pool nothing may initialise HIP in a process that then launches GPU work) — asserted inside self_launch, echoed by rank 0
    assert json.loads(lines[0]) == {"launch_check": True, "n_gpus": 2, "rank_sum": 3.0, "parent_clean": True, "rank_cuda_initialized": False}
    # and without GPUs a real multi-GPU request fails loudly instead of hanging or falling back
    r = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--gpus", "2"], capture_output=True, text=True, env=env, timeout=170)
    if not os.path.isdir("/sys/class/kfd/kfd/topology/nodes"):
        assert r.returncode == 2 and "exposes" in r.stderr


def test_launcher_counts_gpus_from_sysfs_and_imports_torch_only_after_the_launch_decision(tmp_path, monkeypatch):
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py")).read()
    head = src[:src.index("import torch")]
    assert "self_launch(" in head and "torch.cuda" not in head.replace("torch.cuda.device_count() here", "")   # the launch decision precedes the import
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod2", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    for i, simd in enumerate([0, 0, 1024, 1024, 1024]):       # two CPU nodes + three GPUs, the layout of /sys/class/kfd/kfd/topology/nodes
        d = tmp_path / str(i)
        d.mkdir()
        (d / "properties").write_text("cpu_cores_count %d\nsimd_count %d\nmem_banks_count 1\n" % (0 if simd else 64, simd))
    real_listdir, real_open = os.listdir, open
    root = "/sys/class/kfd/kfd/topology/nodes"
    monkeypatch.setattr(os, "listdir", lambda p: real_listdir(str(tmp_path)) if p == root else real_listdir(p))
    import builtins
    monkeypatch.setattr(builtins, "open", lambda p, *a, **k: real_open(str(p).replace(root, str(tmp_path)), *a, **k))
    assert b.kfd_gpu_count() == 3


def test_allreduce_model_is_monotone_and_small_against_the_step():
    import importlib.util
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(repo, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    m = b.allreduce_model(4935990 * 4, 4)
    assert m["n2_ms"] < m["n4_ms"] < m["n8_ms"] < 1.0            # 19.7 MB of fp32 gradients: well under a millisecond on xGMI


def test_compact_bench_line_fits_an_8k_tail_and_keeps_every_roofline_object():
    """the driver keeps an 8 kB tail of stdout.  The compact line (what `python bench.py` prints) must stay well under
    that and end with the evidence: every roofline object (worst fraction first), configs[3], cpu_baseline and the contract's keys."""
    import importlib.util
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_mod3", os.path.join(repo, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    res = json.load(open(os.path.join(repo, "profiles", "r05_bench_n1.json")))       # a real verbose line (round 5)
    res["config0"] = {"workload": "x" * 100, "value": 1.0, "unit": "images/s", "ms": 1.0, "cpu_baseline": {"value": 1.0, "unit": "images/s", "cores": 16, "kind": "port", "sample": "y" * 100}}
    res["config3"]["cpu_baseline"] = {"value": 1.0, "unit": "images/s", "cores": 16, "kind": "port", "sample": "z" * 120}
    c = b.compact_line(res)
    line = json.dumps(c, separators=(",", ":"))
    assert len(line) < 7500, len(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline", "cpu_baseline", "roofline_hbm", "roofline_more", "config3", "config0"):
        assert k in c, k
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in c["roofline"], k
    assert {o["kernel"] for o in c["roofline_more"]} == {o["kernel"] for o in res["roofline_more"]}
    fr = [o["frac"] for o in c["roofline_more"]]
    assert fr == sorted(fr)                                                             # worst first
    tail = line[-5000:]                                                                 # even a 5 kB tail holds the roofline block and configs[3]
    assert '"roofline_more"' in tail and '"config3"' in tail and '"roofline_hbm"' in tail


def test_bench_side_legs_are_opt_in_and_dump_outputs_is_seeded_float_and_capped(tmp_path, monkeypatch):
    """A plain `bench.py` run does only what the headline needs: everything else sits behind --full (off by default).
    --dump-outputs DIR writes both loss tuples and every parameter gradient as float32 .npy files, identical for identical
    inputs, and a fixed seeded sample of every array once the whole dump would exceed its cap."""
    import importlib.util
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_mod4", os.path.join(repo, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = b.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 3
    monkeypatch.setattr("sys.argv", ["bench.py", "--full", "--dump-outputs", str(tmp_path / "x")])
    a = b.parse()
    assert a.full is True and a.dump_outputs == str(tmp_path / "x")
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(64, 32), torch.nn.Linear(32, 3, bias=False))
    m[1].weight.requires_grad_(False)                     # no gradient -> no file
    m(torch.randn(5, 64)).sum().backward()
    out = tuple(tuple(torch.tensor(0.5 * i + j) for j in range(7)) for i in range(2))
    names = sorted(["head0_loss_metrics.npy", "head1_loss_metrics.npy", "grad.0.weight.npy", "grad.0.bias.npy"])
    full_bytes = 4 * (14 + 64 * 32 + 32)
    assert b.dump_outputs(str(tmp_path / "a"), out, m) == (4, full_bytes)
    assert sorted(os.listdir(tmp_path / "a")) == names
    z = {n: np.load(str(tmp_path / "a" / n)) for n in names}
    assert all(v.dtype == np.float32 for v in z.values())
    assert z["head1_loss_metrics.npy"].tolist() == [0.5 + j for j in range(7)]
    np.testing.assert_array_equal(z["grad.0.weight.npy"], m[0].weight.grad.numpy())
    monkeypatch.setattr(b, "DUMP_LIMIT_BYTES", 4096)
    n1 = b.dump_outputs(str(tmp_path / "c1"), out, m)
    n2 = b.dump_outputs(str(tmp_path / "c2"), out, m)
    assert n1 == n2 and n1[1] <= 4096
    for n in names:
        c1, c2 = np.load(str(tmp_path / "c1" / n)), np.load(str(tmp_path / "c2" / n))
        assert c1.dtype == np.float32 and np.array_equal(c1, c2)
    w = np.load(str(tmp_path / "c1" / "grad.0.weight.npy"))
    assert 0 < w.size < 64 * 32 and np.isin(w, m[0].weight.grad.numpy().reshape(-1)).all()
