"""The driver's contract on bench.py's output: the LAST line of stdout is one JSON object of at most 3 KB that
carries the headline keys, `roofline` and `cpu_baseline`; everything else goes to bench_detail.json.  The round-3 line had grown to
28.9 KB and overflowed the driver's ~8 KB tail window, so the driver parsed nothing."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
            "data", "config")


def test_headline_of_the_round3_record_fits():
    """The very record that broke the driver in round 3 (profiles/r3_bench_line_m.json, 28.9 KB) cut down by bench.headline()."""
    import bench
    full = json.loads(open(os.path.join(ROOT, "profiles", "r3_bench_line_m.json")).read().strip().splitlines()[-1])
    assert len(json.dumps(full)) > 20000
    line = json.dumps(bench.headline(full))
    assert len(line) < bench.HEADLINE_MAX_BYTES == 3072
    h = json.loads(line)
    for k in CONTRACT:
        assert k in h, k
    assert h["value"] == full["value"] and h["ms_per_step"] == full["ms_per_step"]
    assert set(h["config"]) == {"workload", "global_batch", "parallelism"}
    assert h["roofline"]["frac"] == full["roofline"]["frac"] and h["roofline"]["kernel"]
    assert h["cpu_baseline"]["value"] == full["cpu_baseline"]["value"] and len(h["cpu_baseline"]["sample"]) <= 160
    for sub in ("config3_bf16", "config5_inference"):
        assert set(h[sub]) == {"value", "ms_per_step", "dtype", "mode", "roofline_frac", "roofline_kernel", "cpu_baseline_value"}
        assert h[sub]["value"] == full[sub]["value"]


def test_headline_survives_failed_sub_records_and_missing_parts():
    import bench
    d = {"metric": "m", "value": 1.0, "unit": "slices/s", "n_gpus": 8, "steps": 2, "warmup": 1, "ms_per_step": 3.0, "higher_is_better": True,
         "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic", "config": {"workload": "w" * 5000, "global_batch": 128,
                                                                                               "parallelism": "dp8"},
         "config3_bf16": {"error": "rc=1: " + "x" * 5000}, "roofline_families": {"a": {"kernels": {str(i): {} for i in range(500)}}}}
    line = json.dumps(bench.headline(d))
    assert len(line) < 3072 and "roofline_families" not in line
    assert json.loads(line)["config3_bf16"]["error"].startswith("rc=1")


@pytest.mark.gpu
def test_bench_last_stdout_line_is_the_small_headline(tmp_path):
    """bench.py --full end to end at a small size: the last stdout line parses, is < 3 KB, carries roofline.frac and cpu_baseline.value,
    the detail file holds the families; stdout carries nothing else."""
    dfile = "bench_detail_test.json"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--size", "64", "--batch", "4", "--steps", "2", "--warmup", "1", "--cpu-threads", "8",
           "--detail-file", dfile, "--full"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=1500, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.strip().splitlines()
    last = lines[-1]
    assert len(last) < 3072, len(last)
    rec = json.loads(last)
    for k in CONTRACT:
        assert k in rec, k
    assert rec["value"] > 0 and rec["steps"] == 2 and rec["warmup"] == 1 and rec["n_gpus"] == 1
    assert 0 < rec["roofline"]["frac"] < 1 and rec["roofline"]["kernel"] and rec["roofline"]["bound"] in ("mfma", "hbm")
    assert rec["cpu_baseline"]["value"] > 0 and rec["cpu_baseline"]["kind"] == "port"
    assert rec["config3_bf16"]["value"] > 0 and rec["config5_inference"]["value"] > 0 and rec["config4_random_masks_n1"]["value"] > 0
    # the pure-fp32-MFMA control next to the X3 headline
    assert rec["dtype"] == "f32 (bf16x3 split)" and rec["config2_fp32_mfma"]["value"] > 0 and rec["config2_fp32_mfma"]["dtype"] == "f32"
    assert "3 warm-up + 5 timed" in rec["cpu_baseline"]["sample"]
    assert rec["config4_random_masks_n1"]["mode"] == "graph"
    assert not any(l.startswith("BENCH_DETAIL") for l in lines)            # the big record goes to stderr and the file
    assert any(l.startswith("BENCH_DETAIL ") for l in out.stderr.splitlines())
    assert "UserWarning" not in out.stderr, out.stderr[-2000:]
    detail = json.load(open(os.path.join(ROOT, dfile)))
    assert "roofline_families" in detail and detail["value"] == rec["value"]
    # round 6 (VERDICT r5 "next" #7): the whole step against its floor in the line, the other configs' CPU baselines in the detail file
    rs = rec["roofline_step"]
    assert rs["bound"] in ("hbm", "mfma") and rs["floor_ms"] > 0 and abs(rs["frac"] - rs["floor_ms"] / rec["ms_per_step"]) < 1e-9 and 0 < rs["frac"] < 1
    assert detail["roofline_step"]["ideal_hbm_gb"] > 0 and detail["roofline_step"]["matrix_floor_ms"] > 0
    other = detail["cpu_baselines_other_configs"]
    assert set(other) == {"config0_bs4_standard_only", "config4_random_masks", "config3_swapped_spatial_channel"}
    assert all(v["value"] > 0 and v["kind"] == "port" and v["cores"] == 8 for v in other.values())
    if rec["roofline"].get("traffic") is not None:                         # the file the figure was read from is named, and exists
        src = rec["roofline"]["traffic_source"]
        assert src.startswith("profiles/") and os.path.exists(os.path.join(ROOT, src.split(":")[0]))
    # the reported kernel is the arg-max of serial time over the profiling ids of the step
    assert rec["roofline"]["kernel"] == detail["kernels_by_serial_time"][0]["kernel"], (rec["roofline"], detail["kernels_by_serial_time"][:3])
    os.remove(os.path.join(ROOT, dfile))


def test_headline_with_every_sub_record_fits():
    """All four sub-records present (config2_fp32_mfma is round 5's) on top of the largest record on file: still < 3 KB."""
    import bench
    full = json.loads(open(os.path.join(ROOT, "profiles", "r3_bench_line_m.json")).read().strip().splitlines()[-1])
    full["config2_fp32_mfma"] = dict(full["config3_bf16"])
    full["config4_random_masks_n1"] = dict(full["config3_bf16"])
    full["roofline"]["traffic_source"] = "s" * 400
    full["roofline_step"] = {"bound": "hbm", "floor_ms": 4.2250000000000005, "frac": 0.29153846153846157, "ideal_hbm_gb": 33.8, "note": "n" * 300}
    line = json.dumps(bench.headline(full))
    assert set(json.loads(line)["roofline_step"]) == {"bound", "floor_ms", "frac"}
    assert len(line) < bench.HEADLINE_MAX_BYTES, len(line)
    assert json.loads(line)["config2_fp32_mfma"]["value"] == full["config3_bf16"]["value"]


def test_gpus_n_without_a_launcher_is_n_ranks_or_an_error():
    """`python bench.py --gpus 2` with WORLD_SIZE unset on a box with no (or too few) GPUs: non-zero exit and a message, never a
    one-rank run labelled n_gpus 1.  (No GPU here: the launcher path refuses before any device is touched.)"""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["HIP_VISIBLE_DEVICES"] = ""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"], capture_output=True,
                         text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode != 0
    assert "--gpus 2" in out.stderr and "GPU(s) visible" in out.stderr, out.stderr[-500:]
    assert not [l for l in out.stdout.splitlines() if l.startswith("{")]


@pytest.mark.gpu
def test_gpus_2_without_a_launcher_runs_two_ranks():
    """--gpus 2 with no torchrun in the command: bench.py starts the two ranks itself (gloo, both on GPU 0) and relays rank 0's line."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    # (--mode eager: the subject is the launcher, not the mode calibration -- two processes time-slicing ONE GPU over gloo run the ~60 steps of
    #  `--mode auto` at 0.1-2 s per step, and about one such run in thirty ended in NaN losses on both ranks, round-5 code included
    #  (tools/debug/r6_dp_flake.sh; never seen in single-process runs or in tests/test_dist_gpu.py, which compares weights bit for bit every run))
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--all-on-device0", "--size", "64", "--batch", "2",
           "--steps", "2", "--warmup", "1", "--mode", "eager", "--no-cpu-baseline", "--no-sub-records", "--detail-file", "bench_detail_test2.json"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=1500, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    rec = json.loads(out.stdout.strip().splitlines()[-1])
    assert rec["n_gpus"] == 2 and rec["config"]["global_batch"] == 4 and rec["config"]["parallelism"] == "dp2" and rec["value"] > 0
    try:
        os.remove(os.path.join(ROOT, "bench_detail_test2.json"))
    except OSError:
        pass


def test_dump_outputs_writes_npy_within_the_cap(tmp_path, monkeypatch):
    """--dump-outputs: one float32 / float64 .npy per array; an array over its share of the cap becomes the same seeded sample every time."""
    import numpy as np
    import torch
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 3 * 4096)
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 512)
    big = torch.arange(10000, dtype=torch.float32)
    arrays = {"losses": torch.tensor([1.0, 2.0], dtype=torch.float64), "mask": torch.tensor([True, False]), "big": big}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in arrays}
    assert a["losses"].dtype == np.float64 and a["losses"].tolist() == [1.0, 2.0]
    assert a["mask"].dtype == np.float32 and a["mask"].tolist() == [1.0, 0.0]
    assert a["big"].dtype == np.float32 and a["big"].shape == (512,) and len(set(a["big"].tolist())) == 512
    assert np.array_equal(a["big"], np.load(tmp_path / "b" / "big.npy"))
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_MAX_BYTES


def test_full_and_dump_outputs_are_options():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "--full" in out.stdout and "--dump-outputs" in out.stdout


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    """A plain run (no --full) times exactly --steps steps, prints the contract keys and none of what --full measures, and with
    --dump-outputs writes the last timed step's losses, masks and updated weights; a second run with the same arguments starts from
    the same inputs and ends with the same outputs."""
    import numpy as np
    recs, dumps = [], []
    for d in ("a", "b"):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--size", "64", "--batch", "4", "--steps", "3", "--warmup", "1", "--mode", "graph",
               "--detail-file", "bench_detail_test_plain.json", "--dump-outputs", str(tmp_path / d)]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-3000:]
        recs.append(json.loads(out.stdout.strip().splitlines()[-1]))
        dumps.append({f[:-4]: np.load(tmp_path / d / f) for f in sorted(os.listdir(tmp_path / d))})
    os.remove(os.path.join(ROOT, "bench_detail_test_plain.json"))
    rec = recs[0]
    for k in CONTRACT:
        assert k in rec, k
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["mode"] == "graph"
    assert rec["ms_per_step"] > 0 and abs(rec["value"] - 4 * 1e3 / rec["ms_per_step"]) <= 1e-6 * rec["value"]
    for k in ("roofline", "cpu_baseline", "config2_fp32_mfma", "config3_bf16", "config5_inference", "config4_random_masks_n1", "latent_mask_hbm_frac"):
        assert k not in rec, k
    a, b = dumps
    assert a["losses"].dtype == np.float64 and a["losses"].shape == (8,) and np.isfinite(a["losses"]).all()
    assert {"mask_image", "mask_seg"} <= set(a) and len([k for k in a if k.startswith("weights_")]) == 5
    assert all(v.dtype in (np.float32, np.float64) for v in a.values()) and sum(v.nbytes for v in a.values()) <= 64 << 20
    assert set(a) == set(b)
    for k in a:
        assert np.allclose(a[k], b[k], rtol=1e-4, atol=1e-6), k
