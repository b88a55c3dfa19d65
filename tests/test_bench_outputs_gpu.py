"""bench.py's plain run and `--dump-outputs DIR`: exactly --steps timed steps in one region, none of the `--full` legs, and
the outputs of the last timed step written as float64 .npy files that are the same from run to run (a long column as a
fixed seeded sample of rows).  The second test times a run in spans (the device holding fewer rounds than the run asks
for) and checks that it computes what the single region computes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, STEPS, WARMUP = 200_000, 4, 2  # 600,000 votes per step: vote_status is written as a sample of rows


def _bench(args, prelude=""):
    code = ("import sys; sys.path.insert(0, %r); import bench, torch; %s"
            "sys.argv = ['bench.py'] + %r; sys.exit(bench.main() or 0)" % (ROOT, prelude, list(args)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_plain_run_dumps_the_last_step(hip_lib, tmp_path):
    common = ["--gpus", "1", "--groups", str(G), "--steps", str(STEPS), "--warmup", str(WARMUP)]
    a = _bench(common + ["--dump-outputs", str(tmp_path / "a")])
    assert a["steps"] == STEPS and a["ms_per_step"] > 0 and a["value"] > 0
    assert a["ms_per_step_spread"]["timed_regions"] == 1
    assert a["roofline"] is None and a["end_to_end"] is None and a["cpu_baseline"] is None and a["parity_checked"] is None
    out = _load(tmp_path / "a")
    assert sum(os.path.getsize(tmp_path / "a" / (k + ".npy")) for k in out) <= 64 << 20
    assert all(v.dtype == np.float64 for v in out.values())
    assert out["n_decided"].tolist() == [G]
    for k in ("slot", "bnum", "bcoord", "median_cp", "status"):
        assert out["propose_" + k].shape == (G,)
    for k in ("gidx", "slot", "bnum", "bcoord", "median_cp", "kind"):
        assert out["decided_" + k].shape == (G,)
    assert out["vote_status"].shape == (1 << 19,)
    # the last timed step is round WARMUP + STEPS - 1: every group proposed and decided slot WARMUP + STEPS
    assert (out["propose_slot"] == WARMUP + STEPS).all() and (out["propose_status"] == 0).all()
    assert (out["decided_slot"] == WARMUP + STEPS).all() and (out["decided_kind"] == 1).all()
    assert sorted(out["decided_gidx"].astype(np.int64).tolist()) == list(range(G))
    # the same arguments, the same inputs: the same outputs
    _bench(common + ["--dump-outputs", str(tmp_path / "b")])
    again = _load(tmp_path / "b")
    assert sorted(again) == sorted(out) and all(np.array_equal(out[k], again[k]) for k in out)


def test_run_timed_in_spans_computes_the_same(hip_lib, tmp_path):
    """--pool 2 and a device that reports room for four rounds' (slot, max_cp) columns: warm-up and the timed steps run in
    spans of four rounds, the columns refilled between them.  run_timed's own checks (G decisions per round, the last
    round's slot) hold, and the outputs equal those of the same run in one region."""
    g, steps = 100_000, 10
    common = ["--gpus", "1", "--groups", str(g), "--steps", str(steps), "--warmup", "3", "--pool", "2"]
    small = "torch.cuda.mem_get_info = lambda *a: (%d, %d); " % ((2 * 4 * 8 * 3 * g,) * 2)
    spans = _bench(common + ["--dump-outputs", str(tmp_path / "spans")], prelude=small)
    one = _bench(common + ["--dump-outputs", str(tmp_path / "one")])
    assert spans["steps"] == one["steps"] == steps and spans["ms_per_step"] > 0
    a, b = _load(tmp_path / "spans"), _load(tmp_path / "one")
    assert a["n_decided"].tolist() == [g] and (a["decided_slot"] == 3 + steps).all()
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
