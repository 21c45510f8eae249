"""bench.py's rank launcher (CPU): `python bench.py --gpus N` outside a
torch.distributed launch must start N rank processes (one per GPU, the
reference's Lightning DDP over all devices, main.py:108-119) before anything
touches the GPU; under torchrun, WORLD_SIZE must equal --gpus.  Also the
benchmark's own helpers (PMC records, --dump-outputs) and, on the GPU, what a
plain run prints and writes."""
import importlib.util
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_single_gpu_runs_in_process():
    b = _bench()
    assert b.launch_plan([], {}) is None
    assert b.launch_plan(["--gpus", "1", "--steps", "2"], {}) is None


def test_multi_gpu_spawns_ranks():
    b = _bench()
    argv = ["--gpus", "8", "--steps", "5", "--warmup", "2"]
    cmd = b.launch_plan(argv, {})
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=8" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert any(c.startswith("--master-port=") and int(c.split("=")[1]) > 0 for c in cmd)
    assert cmd[-len(argv) - 1] == os.path.join(REPO, "bench.py")
    assert cmd[-len(argv):] == argv  # the ranks see the same --gpus and see WORLD_SIZE


def test_ranks_under_torchrun_run_in_process():
    b = _bench()
    assert b.launch_plan(["--gpus", "4"], {"WORLD_SIZE": "4"}) is None


def test_world_size_mismatch_refused():
    b = _bench()
    with pytest.raises(SystemExit) as e:
        b.launch_plan(["--gpus", "8"], {"WORLD_SIZE": "2"})
    assert e.value.code == 2
    # end to end: refused before torch or the package is imported
    env = dict(os.environ, WORLD_SIZE="1")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2"], env=env,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "refusing" in r.stderr


def test_launcher_starts_children_and_returns_their_status(tmp_path):
    """The launch path never imports torch in the parent: a fake
    torch.distributed.run on PYTHONPATH records its argv and exits 3; bench.py
    must exit with that status."""
    pkg = tmp_path / "torch" / "distributed"
    pkg.mkdir(parents=True)
    (tmp_path / "torch" / "__init__.py").write_text("")
    (pkg / "__init__.py").write_text("")
    rec = tmp_path / "argv.txt"
    (pkg / "run.py").write_text(f"import sys\nopen({str(rec)!r}, 'w').write(' '.join(sys.argv[1:]))\n"
                                "sys.exit(3)\n")
    env = dict(os.environ, PYTHONPATH=str(tmp_path))
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "1"],
                       env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 3, r.stderr
    got = rec.read_text()
    assert "--nproc-per-node=2" in got and got.endswith("--gpus 2 --steps 1")


def test_pmc_fields_tied_to_kernel_sources(tmp_path, monkeypatch):
    """a committed PMC record's counters are printed only while
    the kernel's sources are the ones it was collected on (buildinfo digest);
    otherwise load_pmc returns None with the reason."""
    import json
    b = _bench()
    from tmr_amd import buildinfo
    rec = {"hbm_bytes_per_launch": 1.0, "source_digest": buildinfo.source_digest("heads")}
    p = tmp_path / "pmc.json"
    p.write_text(json.dumps({"round": "t", "configs": {"B": {"heads": rec}}}))
    monkeypatch.setattr(b, "PMC_FILE", str(p))
    got, why = b.load_pmc("B", "heads")
    assert why is None and got["hbm_bytes_per_launch"] == 1.0 and "round t" in got["source"]
    rec["source_digest"] = "0" * 16
    p.write_text(json.dumps({"round": "t", "configs": {"B": {"heads": rec}}}))
    got, why = b.load_pmc("B", "heads")
    assert got is None and "other kernel sources" in why
    assert b.load_pmc("C", "heads") == (None, "no PMC record for this config")


def test_source_digest_ignores_comments_only():
    """The digest hashes the code: a comment or layout edit keeps it, any
    token change moves it."""
    from tmr_amd import buildinfo
    a = b"int f(int x) { // twice\n  return 2 * x; /* doubled */ }\n"
    assert buildinfo._code("k.hip", a) == buildinfo._code("k.hip", b"int f(int x) {\n return 2 * x; }")
    assert buildinfo._code("k.hip", a) != buildinfo._code("k.hip", a.replace(b"2 * x", b"3 * x"))
    mk = b"# flags\nHIPFLAGS = -O3\n"
    assert buildinfo._code("Makefile", mk) == buildinfo._code("Makefile", b"HIPFLAGS = -O3")
    assert buildinfo._code("Makefile", mk) != buildinfo._code("Makefile", b"HIPFLAGS = -O2")


def test_committed_pmc_records_match_this_tree():
    """Every record of the committed profiles/pmc_by_config.json was collected
    on the kernel sources of this tree (so every bench line's traffic /
    mfma_busy_pmc is live): a kernel edit without re-running
    profiles/gpu_pmc.sh turns this red."""
    import json
    from tmr_amd import buildinfo
    d = json.load(open(os.path.join(REPO, "profiles", "pmc_by_config.json")))
    stale = []
    for cfg, roles in d["configs"].items():
        for role, rec in roles.items():
            if isinstance(rec, dict) and rec.get("source_digest") != buildinfo.source_digest(role):
                stale.append(f"{cfg}/{role}")
    assert set(d["configs"]) >= {"A", "B", "C", "D", "E"}
    assert not stale, f"PMC records from other kernel sources: {stale} (re-run profiles/gpu_pmc.sh)"


def _detections(counts, seed=3):
    import torch
    g = torch.Generator().manual_seed(seed)
    L = [torch.rand(n, 2, generator=g) for n in counts]
    Bx = [torch.rand(n, 4, generator=g) for n in counts]
    R = [torch.rand(n, 2, generator=g) for n in counts]
    return L, Bx, R


def test_dump_outputs_writes_the_detections(tmp_path):
    """--dump-outputs: the per-image lists of the last step, image after image,
    as float32 .npy files with the rows per image beside them."""
    import numpy as np
    import torch
    b = _bench()
    counts = [5, 0, 7]
    L, Bx, R = _detections(counts)
    d = tmp_path / "out" / "dir"  # created on demand
    b.dump_outputs(str(d), L, Bx, R)
    assert sorted(os.listdir(d)) == ["boxes.npy", "counts.npy", "logits.npy", "refs.npy"]
    got = {n: np.load(d / (n + ".npy")) for n in ("logits", "boxes", "refs", "counts")}
    assert all(v.dtype == np.float32 for v in got.values())
    assert got["counts"].tolist() == counts
    assert got["logits"].shape == (12, 2) and got["boxes"].shape == (12, 4) and got["refs"].shape == (12, 2)
    assert np.array_equal(got["logits"], torch.cat(L).numpy())
    assert np.array_equal(got["boxes"], torch.cat(Bx).numpy())
    assert np.array_equal(got["refs"], torch.cat(R).numpy())


def test_dump_outputs_samples_above_the_size_limit(tmp_path, monkeypatch):
    """Above the limit the same seeded sample of rows is written every time,
    with the rows' indices, and the files together stay under the limit."""
    import numpy as np
    import torch
    b = _bench()
    L, Bx, R = _detections([300, 500])
    monkeypatch.setattr(b, "DUMP_MAX_BYTES", 16384)
    for name in ("a", "b"):
        b.dump_outputs(str(tmp_path / name), L, Bx, R)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["boxes.npy", "counts.npy", "logits.npy", "refs.npy", "sample_rows.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 16384
    for f in files:
        assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes()
    rows = np.load(tmp_path / "a" / "sample_rows.npy")
    assert rows.dtype == np.float64 and 0 < len(rows) < 800 and np.all(np.diff(rows) > 0)
    assert np.load(tmp_path / "a" / "counts.npy").tolist() == [300, 500]  # of the whole output
    assert np.array_equal(np.load(tmp_path / "a" / "boxes.npy"), torch.cat(Bx).numpy()[rows.astype(int)])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_outputs(tmp_path):
    """A plain `bench.py --gpus 1 --steps N --warmup W` times N steps and
    prints the headline fields only (nothing that needs a run of its own);
    --dump-outputs writes the last step's detections."""
    import json
    import numpy as np
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2",
                        "--warmup", "1", "--config", "A", "--dump-outputs", str(tmp_path / "o")],
                       capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["steps"] == 2 and out["warmup"] == 1 and out["unit"] == "images/s"
    assert out["higher_is_better"] is True and out["dtype"] == "fp32" and out["metric"]
    assert out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(1e3 / out["ms_per_step"], rel=1e-3)  # config A: one image per step
    for k in ("roofline", "roofline_xcorr", "bare_loop", "cpu_baseline"):
        assert k not in out
    counts = np.load(tmp_path / "o" / "counts.npy")
    boxes = np.load(tmp_path / "o" / "boxes.npy")
    assert counts.shape == (1,) and counts[0] >= 1 and boxes.shape == (int(counts[0]), 4)
    assert out["config"]["mean_kept_per_image"] == round(float(counts.mean()), 1)
    assert np.isfinite(boxes).all() and np.load(tmp_path / "o" / "logits.npy").shape == (int(counts[0]), 2)


def test_frac_guard_nulls_fractions_above_one():
    b = _bench()
    out = {"roofline": {"frac": 0.2, "executed_frac": 1.3, "nested": {"x_frac": 2.0, "n": 5}}, "frac": 0.9}
    hits = b.guard_fracs(out)
    assert out["roofline"]["executed_frac"] is None and out["roofline"]["nested"]["x_frac"] is None
    assert out["roofline"]["frac"] == 0.2 and out["frac"] == 0.9 and out["roofline"]["nested"]["n"] == 5
    assert sorted(hits) == ["roofline.executed_frac=1.3", "roofline.nested.x_frac=2.0"]
