"""GPU tests of bench.py's single-rank lines other than the driver's default:
every workload the bench can time carries its own oracle windows (VERDICT r05
item 3 applies to every record, not only the N > 1 ones), and the default
invocation also runs in f32 with all its sub-records.  Small sizes; one bench
process per case (the test runner itself runs once)."""
import json
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]


def _bench(*args, expect_rc=0):
    cmd = [sys.executable, str(ROOT / "bench.py"), "--full", "--steps", "3", "--warmup", "1",
           "--no-cpu-baseline", "--buffer-sets", "2", *args]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(ROOT))
    assert r.returncode == expect_rc, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.parametrize("args,windows", [
    (("--workload", "tree64", "--sites", "4099"), 63),
    (("--workload", "tree64", "--tips", "--sites", "4099"), 63),
    (("--workload", "tree64", "--fuse", "2", "--sites", "4099"), 63),
    (("--workload", "protein", "--sites", "4099"), 1),
    (("--workload", "protein", "--exact", "--sites", "4099"), 1),
    (("--workload", "protein", "--valu", "--sites", "4099"), 1),
    (("--workload", "protein", "--tips", "--sites", "4099"), 1),
    (("--workload", "protein", "--dtype", "f32", "--sites", "4099"), 1),
    (("--workload", "nodes512", "--nodes", "6", "--sites", "4099"), 6),
    (("--workload", "nodes512", "--nodes", "70", "--per-launch", "32", "--sites", "4099"), 70),
    (("--workload", "node", "--lanes", "1", "--sites", "4099"), 1),
    (("--workload", "node", "--launch", "bound", "--sites", "4099"), 1),
    (("--workload", "protein", "--lanes", "1", "--sites", "4099"), 1),
    (("--workload", "protein", "--launch", "bound", "--valu", "--sites", "4099"), 1),
])
def test_workload_lines_carry_oracle_windows(args, windows):
    d = _bench(*args)
    c = d["config"]
    assert d["check"] == "ok"
    assert c["check_windows"] == windows and c["windows_mismatched"] == 0
    assert c["region_start"] == "single rank"
    assert d["value"] > 0 and d["roofline"]["frac"] > 0
    # node / protein steps alternate over 2 streams unless --lanes 1
    want = 1 if "--lanes" in args or args[1] == "tree64" else 2
    assert c["lanes"] == want == d["roofline"]["lanes"]


def test_default_invocation_f32_with_every_sub_record():
    """The default command in f32: the node line and its four sub-records,
    each oracle-checked (tree64 against the reference's plf() composed per
    node in its float build, or the oracle's traversal)."""
    d = _bench("--dtype", "f32", "--sites", "65536", "--nodes", "4")
    c = d["config"]
    assert d["check"] == "ok" and d["dtype"] == "f32"
    assert c["check_windows"] == 1 and c["windows_mismatched"] == 0
    for k, n in (("nodes512", 4), ("tree64", 63)):
        assert c[k]["check"] == "ok" and c[k]["check_windows"] == n and c[k]["windows_mismatched"] == 0
        assert c[k]["dtype"] == "f32"
    for p in (c["protein"], c["protein"]["exact"]):
        assert p["check"] == "ok" and p["check_windows"] == 1 and p["dtype"] == "f32"
        assert p["lanes"] == 2
    assert c["lanes"] == 2 and c["nodes512"]["lanes"] == 2 and c["tree64"]["lanes"] == 1
    assert "valu_fma" not in c["protein"]  # the VALU FMA form is f64 only


def test_corrupted_single_rank_line_fails():
    """--corrupt-rank 0 at one rank: the node line and every sub-record fail
    their windows, the command exits 3."""
    d = _bench("--sites", "65536", "--nodes", "2", "--corrupt-rank", "0", expect_rc=3)
    c = d["config"]
    assert d["check"].startswith("CHECK_FAILED")
    assert c["windows_mismatched"] == 1
    for k in ("nodes512", "tree64"):
        assert c[k]["check"] == "CHECK_FAILED" and c[k]["windows_mismatched"] == 1
    for p in (c["protein"], c["protein"]["valu_fma"], c["protein"]["exact"]):
        assert p["windows_mismatched"] == 1 and p["check"] == "CHECK_FAILED"


def test_sweep_small_sites_one_and_two_lanes():
    """bench.py --sweep: per-call cost at small site counts on one stream and
    over two lanes (independent outputs), every path's outputs checked."""
    cmd = [sys.executable, str(ROOT / "bench.py"), "--sweep", "--sweep-sites", "1,1000,65537"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(ROOT))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    d = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert d["check"] == "ok" and [row["sites"] for row in d["rows"]] == [1, 1000, 65537]
    for row in d["rows"]:
        assert row["check"] == "ok" and 0 < row["graph_two_lanes_us_per_call"] and 0 < row["graph_us_per_call"]


def test_plain_run_is_lean_and_dumps_the_last_step(oracle, tmp_path):
    """A plain run (no --full) times exactly --steps steps, checks and measures
    nothing else, and --dump-outputs writes what the last timed step computed:
    step warmup + steps - 1 = 4 ran on buffer set 4 % 3 = 1, whose inputs are
    the host_mem protocol's of seed SEED + 1, so x3, the scaler bytes and the
    scaler sum equal the oracle's bit for bit."""
    import numpy as np

    sys.path.insert(0, str(ROOT))
    import bench

    n = 4099
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
           "--buffer-sets", "3", "--sites", str(n), "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(ROOT))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 2 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["metric"] == bench.METRIC and d["unit"] == "sites/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f64" and d["value"] == pytest.approx(n / (d["ms_per_step"] * 1e-3))
    assert d["check"].startswith("not run") and d["cpu_baseline"] is None
    assert "host_buffers" not in d and "traffic" not in d["roofline"]
    assert "frac_second_region" not in d["roofline"] and d["roofline"]["frac"] > 0
    assert not {"nodes512", "tree64", "protein", "check_windows", "lnl_per_rank"} & set(d["config"])
    h = oracle.gen_hostmem(n, np.float64, bench.SEED + 1)
    e3, esc, einc = oracle.plf(h["x1"], h["x2"], h["EV"], h["left"], h["right"], h["wgt"])
    got = {p.name: np.load(p) for p in (tmp_path / "out").iterdir()}
    assert sorted(got) == ["scaler.npy", "scaler_sum.npy", "x3.npy"]
    assert got["x3.npy"].dtype == np.float64 and got["scaler.npy"].dtype == np.float32
    assert np.array_equal(got["x3.npy"].view(np.uint64), e3.view(np.uint64))
    assert np.array_equal(got["scaler.npy"], esc.astype(np.float32))
    assert got["scaler_sum.npy"].tolist() == [float(einc)]
    assert d["dumped_outputs"]["x3"] == [[16 * n], "float64"]
