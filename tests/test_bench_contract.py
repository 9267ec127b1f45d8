"""bench.py's one-line JSON contract on one GPU (a small, fast configuration)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def check_dumped_outputs(out, steps, warmup, nsplit):
    """--dump-outputs wrote the state a begin_timestep, a warm-up call and the timed call leave on bench.py's
    default workload (bitwise: the same library, the same calls), a larger array at bench.py's seeded sample"""
    sys.path.insert(0, ROOT)
    import bench
    import numpy as np
    import pamg
    import pamg.solver as P
    s = pamg.SemiImplicitIterative(pamg.Mesh.read(bench.MESH), nsplit, 3, n_smooth=4, solver=3, arith=1, fused=3)
    s.begin_timestep()
    s.vcycle(warmup)
    s.vcycle(steps)
    s.synchronize()
    names = sorted(f"{n}_L{l}.npy" for l in (1, 2, 3) for n in ("tnew", "res"))
    assert sorted(os.listdir(out)) == names
    total = 0
    for l in (1, 2, 3):
        for n, what in (("tnew", P.TNEW), ("res", P.RESIDUAL)):
            got = np.load(os.path.join(out, f"{n}_L{l}.npy"))
            want = s.get(what, l).reshape(-1, order="F")
            if want.size > bench.DUMP_SAMPLE:
                want = want[np.random.default_rng(bench.DUMP_SEED).integers(0, want.size, bench.DUMP_SAMPLE)]
            assert got.dtype == np.float64 and got.shape == want.shape
            assert np.array_equal(got, want), (n, l)
            total += got.nbytes
    assert np.abs(np.load(os.path.join(out, "tnew_L1.npy"))).max() > 0
    assert total <= 64 << 20
    s.close()


@pytest.mark.gpu
def test_bench_prints_the_contract_line(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "4", "--warmup", "2",
                        "--nsplit", "3", "--no-extra", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    # a plain run (no --full) measures nothing beside its headline figure
    assert d["cpu_baseline"] is None and d["time_loop"] is None and d["roofline_hbm_smoother"] is None
    assert "sweep_assembled" not in d["extra"] and "op1" not in d["extra"]
    check_dumped_outputs(tmp_path / "out", steps=4, warmup=2, nsplit=3)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
              "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 4 and d["warmup"] == 2
    assert d["unit"] == "V-cycles/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["value"] > 0 and abs(d["ms_per_step"] - 1e3 / d["value"]) < 1e-3 * max(1.0, 1e3 / d["value"])
    assert "workload" in d["config"]
    rf = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in rf, k
    # the resident call (default) is fp64-issue-bound: its roofline is fp64 TFLOP/s against the 78.6
    # TFLOP/s peak; the other schedules' launches are HBM-bound
    if rf["bound"] == "fp64-valu":
        assert rf["unit"] == "TFLOP/s" and rf["peak"] == 78.6 and rf["cycles_per_launch"] == 4
    else:
        assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    assert 0 < rf["frac"] < 1.0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3


def test_pmc_traffic_is_reported_only_for_the_build_it_was_measured_on(tmp_path, monkeypatch):
    """bench.py reads roofline.traffic from the committed rocprofv3 PMC summary only when the
    summary's kernel-source digest (scripts/pmc_summary.py) matches the current sources"""
    sys.path.insert(0, ROOT)
    import bench
    import importlib.util
    spec = importlib.util.spec_from_file_location("pmc_summary", os.path.join(ROOT, "scripts", "pmc_summary.py"))
    ps = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ps)
    assert ps.source_digest() == bench.source_digest()
    prof = tmp_path / "profiles"
    prof.mkdir()
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    # the digest itself is computed over the real tree
    monkeypatch.setattr(bench, "source_digest", lambda: ps.source_digest())
    rec = {"n_split": 5, "levels": 3, "hbm_bytes_per_launch": 1.0e9, "commit": "abc1234",
           "source_digest": ps.source_digest()}
    (prof / "pmc_vcycle_res.json").write_text(json.dumps(rec))
    info = {}
    assert bench.pmc_traffic("vcycle_res", 5, 3, info) == 1.0e9
    assert info["source_matches_build"] is True and info["commit"] == "abc1234"
    assert bench.pmc_traffic("vcycle_res", 6, 3) is None   # another configuration
    rec["source_digest"] = "0" * 16                          # measured on other kernels: stale
    (prof / "pmc_vcycle_res.json").write_text(json.dumps(rec))
    info = {}
    assert bench.pmc_traffic("vcycle_res", 5, 3, info) is None
    assert info["source_matches_build"] is False
    assert bench.pmc_traffic("vcycle_pipe", 5, 3) is None    # no summary at all
