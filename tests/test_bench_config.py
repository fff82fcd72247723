"""bench.py runs the BASELINE.json configurations it claims: shard sizes per GPU count, workload names, and the
hash that ties a committed PMC profile to the kernel sources (no GPU needed); and what a plain run does and dumps
(one test on the GPU)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_items_per_gpu_follow_the_baseline_configs():
    # configs[1]: 2^20 single on one GPU; N = 2, 4 keep 2^20 per GPU (weak scaling, N = 1 equals the headline);
    # configs[3]: 2^24 single over 8 GPUs = 2^21 per GPU
    assert [bench.items_per_gpu("single", w, None) for w in (1, 2, 4, 8)] == [1 << 20, 1 << 20, 1 << 20, 1 << 21]
    for s in ("double", "vargen"):        # configs[2], configs[4]: 2^20 per GPU at every N
        assert [bench.items_per_gpu(s, w, None) for w in (1, 2, 4, 8)] == [1 << 20] * 4
    assert bench.items_per_gpu("single", 8, 12) == 1 << 12
    assert 8 * bench.items_per_gpu("single", 8, None) == 1 << 24


def test_workload_names_cite_the_config():
    cfgs = json.load(open(os.path.join(ROOT, "BASELINE.json")))["configs"]
    assert "2^24 single" in cfgs[3] and "8 MI355X" in cfgs[3]
    assert "configs[3]" in bench.workload_name("single", 1 << 21, 8) and "2^24" in bench.workload_name("single", 1 << 21, 8)
    assert "configs[1]" in bench.workload_name("single", 1 << 20, 1)
    assert "configs[2]" in bench.workload_name("double", 1 << 20, 1)
    assert "configs[4]" in bench.workload_name("vargen", 1 << 20, 4)
    assert "override" in bench.workload_name("single", 1 << 12, 1)


def test_committed_pmc_counters_are_only_quoted_for_the_code_they_were_measured_on(tmp_path, monkeypatch):
    h = bench.csrc_hash()
    assert len(h) == 64 and h == bench.csrc_hash()
    prof = tmp_path / "profiles"
    prof.mkdir()
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    monkeypatch.setattr(bench, "csrc_hash", lambda: h)
    rec = {"csrc_sha256": h, "schemes": {"single": {"items": 1 << 20, "hbm_bytes_per_launch": 1.0,
                                                    "valu_wave_instr_per_launch": 2.0, "source": "x"}}}
    (prof / "pmc_latest.json").write_text(json.dumps(rec))
    assert bench.committed_pmc("single", 1 << 20)["valu_wave_instr_per_launch"] == 2.0
    assert bench.committed_pmc("single", 1 << 21) is None and bench.committed_pmc("double", 1 << 20) is None
    rec["csrc_sha256"] = "0" * 64                      # profile of other code: nothing is quoted
    (prof / "pmc_latest.json").write_text(json.dumps(rec))
    assert bench.committed_pmc("single", 1 << 20) is None


def test_host_info_names_the_cpu():
    info = bench.host_info()
    assert info["nproc"] >= info["affinity_cores"] >= 1 and "cpu_model" in info


def test_thread_choice_prefers_the_fastest_probe():
    info = {"affinity_cores": 256, "cgroup_cpu_quota_cores": None}
    rates = {128: 17000.0, 64: 19000.0, 32: 21000.0, 16: 21700.0, 8: 11000.0}
    t, r, seen = bench.pick_threads(lambda k: rates[k], info, 128)
    assert (t, r) == (16, 21700.0) and sorted(seen) == [8, 16, 32, 64, 128]
    info = {"affinity_cores": 256, "cgroup_cpu_quota_cores": 16.0}
    t, _, seen = bench.pick_threads(lambda k: 1000.0 * k, info, 128)
    assert t == 16 and max(seen) == 16


def test_dumped_outputs_are_exact_floats_and_bounded(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_VALUES", 1 << 12)
    status = np.arange(1 << 13, dtype=np.uint8) % 4
    tally = np.array([5, 0, 3, (1 << 40) + 1], np.int64)
    keys = (np.arange(50 * 64) % 251).astype(np.uint8).reshape(50, 64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"status": status, "tally": tally, "keys": keys})
    got = {f.name: np.load(f) for f in (tmp_path / "a").iterdir()}
    assert sorted(got) == ["keys.npy", "status.npy", "status_rows.npy", "tally.npy"]
    assert got["tally.npy"].dtype == np.float64 and got["tally.npy"].tolist() == tally.tolist()
    assert got["keys.npy"].dtype == np.float32 and (got["keys.npy"] == keys).all()
    rows = got["status_rows.npy"].astype(np.int64)            # a sample of the larger output, rows in order, no repeats
    assert len(rows) == 1 << 12 and (np.diff(rows) > 0).all()
    assert got["status.npy"].dtype == np.float32 and (got["status.npy"] == status[rows]).all()
    for f, a in got.items():                                  # the same sample every time
        assert (np.load(tmp_path / "b" / f) == a).all()


@pytest.mark.gpu
def test_plain_run_times_the_headline_and_dumps_what_it_computed(tmp_path):
    """A plain run: the contract's keys for the K timed steps of the headline only, and the statuses and tally of its last
    step, the same in two runs with the same arguments."""
    n, dumps = 1 << 14, []
    for d in ("a", "b"):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
               "--log2-items-per-gpu", "14", "--dump-outputs", str(tmp_path / d)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert p.returncode == 0, p.stderr[-3000:]
        lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        line = json.loads(lines[0])
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
        assert line["metric"] == "Schnorr verifications/sec" and line["unit"] == "verifications/s" and line["higher_is_better"] is True
        assert line["config"]["items_per_gpu"] == n and all(line["bit_exact"].values())
        assert not {"schemes", "cpu_baseline", "unique_keys", "multisig", "small_host_calls"} & set(line)
        assert line["full_record"] is None
        dumps.append({f.name: np.load(f) for f in (tmp_path / d).iterdir()})
    a, b = dumps
    assert sorted(a) == ["status.npy", "tally.npy"] and a["status.npy"].shape == (n,)
    assert a["tally.npy"].tolist() == [float((a["status.npy"] == k).sum()) for k in range(4)]
    assert all((a[f] == b[f]).all() for f in a)
