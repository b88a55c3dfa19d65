"""The mixed-op fuzz of tests/parity_common.py on every back end of the entry points, one cell per back end.

test_parity_gpu.py's fuzz sends at most 300 records per call: accept replies of up to 1,024 votes go to k_ar_tiny, and
the other back ends only ever see stream-shaped batches.  Here each cell sets the switches that pick its back end
(read when the HIP engine is created, so they are set before it is) and asserts with gpx_profile_read which kernels
ran and which did not:

  partition   GPX_SAR_MAX_N=0, GPX_AR_TILES=0: k_hist + k_scatter_ar16 + k_bucket_ar16 for kmax 3, 5, 8 and 16
  tiles       GPX_SAR_MAX_N=0, batches of 1,025 records or more: k_scatter_tiles
  runs hint   GPX_SAR_MAX_N=0, GPX_TRY_RUNS=1: k_runs_check, the partition behind it
  big batches unordered ACCEPT / COMMIT batches past 65,536 records (k_order_check + the partition), with buckets
              that hold more records than the LDS staging can
  wide        GPX_BUCKET_SHIFT=11 and 12: buckets of 2,048 / 4,096 groups on 1,024 threads (k_scatter_ac,
              k_bucket_accept, k_bucket_commit, k_emit_runs, k_bucket_propose, k_bucket_prepare), hot groups on
              shared threads; the election fuzz, the request batcher and accept-reply packing under the same switch

Windows 4, 8 and 32 are spread over the cells; every cell asserts that ACCEPTs and commits were each refused with
GPX_S_WINDOW at least once, and most that proposals were too.  The cells are defined in geometry_common.CELLS;
test_geometry_model.py runs the same cells oracle against oracle on the CPU."""
import numpy as np
import pytest

from gigapaxos_amd import S_WINDOW
from tests import election_common as E
from tests import host_rows_common as H
from tests.geometry_common import geometry, hot_set, CELLS, run_cell

pytestmark = pytest.mark.gpu

SWITCHES = ("GPX_AR_TILES", "GPX_TRY_RUNS", "GPX_SAR_MAX_N", "GPX_BUCKET_SHIFT", "GPX_TILE_T", "GPX_TILE_NT")


def _env(monkeypatch, env):
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def _cell(hip_lib, oracle_lib, monkeypatch, name, **kw):
    c = CELLS[name]
    _env(monkeypatch, c["env"])
    seen, ran = run_cell(hip_lib, oracle_lib, c, profile=True, **kw)
    if not kw:
        for op in c["refused"]:
            assert S_WINDOW in seen[op], (name, op, seen)
    return seen, ran


def _names(prefix):
    return [n for n in CELLS if n.startswith(prefix)]


@pytest.mark.parametrize("name", _names("partition-"))
def test_partition_pipeline_for_accept_replies(hip_lib, oracle_lib, monkeypatch, name):
    """kmax 3 -> k_bucket16<AR, 4>, 5 -> k_bucket_ar16_k5, 8, 16: the 16-byte partition pipeline for every call."""
    _, ran = _cell(hip_lib, oracle_lib, monkeypatch, name)
    assert {"k_hist", "k_scatter_ar16", "k_bucket_ar16", "k_emit_dec16"} <= ran, sorted(ran)
    assert "k_ar_tiny" not in ran and "k_scatter_tiles" not in ran, sorted(ran)


@pytest.mark.parametrize("name", _names("tiles-"))
def test_tiled_front_end(hip_lib, oracle_lib, monkeypatch, name):
    _, ran = _cell(hip_lib, oracle_lib, monkeypatch, name)
    assert {"k_scatter_tiles", "k_emit_dec16"} <= ran and "k_ar_tiny" not in ran, sorted(ran)
    assert "k_scatter_ar16" not in ran, sorted(ran)


@pytest.mark.parametrize("name", _names("runs-"))
def test_runs_hint_in_front(hip_lib, oracle_lib, monkeypatch, name):
    _, ran = _cell(hip_lib, oracle_lib, monkeypatch, name)
    assert any(k.startswith(("k_runs_check", "k_ar_runs")) for k in ran) and "k_ar_tiny" not in ran, sorted(ran)
    assert "k_scatter_tiles" in ran or "k_scatter_ar16" in ran, sorted(ran)


def test_unordered_accept_commit_batches_past_the_fused_launch(hip_lib, oracle_lib, monkeypatch):
    """Shuffled ACCEPT / COMMIT batches of more than 65,536 records over 1,024 groups (4 buckets of 256): every bucket
    gets more records than even the largest LDS staging of the 16-byte partition holds, so the per-bucket kernels
    regroup them in global memory."""
    c = CELLS["big-accept-commit-k3-w8"]
    geo = geometry(c["G"], c["kmax"])
    # a batch of min_batch records drawn uniformly over G groups: every bucket ~min_batch / nbk records
    assert c["min_batch"] // geo["nbk"] > 1.2 * geo["lds16_hw"], geo
    seen, ran = _cell(hip_lib, oracle_lib, monkeypatch, "big-accept-commit-k3-w8")
    assert seen["accept"] and seen["commit"], seen
    assert {"k_order_check", "k_scatter_ac16", "k_bucket_accept16", "k_bucket_commit16", "k_emit_runs16"} <= ran, sorted(ran)
    assert "k_ac_small" not in ran, sorted(ran)


@pytest.mark.parametrize("name", _names("wide-"))
def test_buckets_wider_than_a_workgroup(hip_lib, oracle_lib, monkeypatch, name):
    """GPX_BUCKET_SHIFT=11 / 12: what every table past 4 M groups runs (buckets of 2,048 / 4,096 groups on 1,024
    threads, ac16 off), cheaply and for many steps.  The fuzzed rows include lanes l, l + 1024, ... of one bucket."""
    c = CELLS[name]
    geo = geometry(c["G"], c["kmax"], c["shift"])
    assert geo["shift"] == c["shift"] and geo["bucket_threads"] == 1024 and not geo["ac16"], geo
    _, place = hot_set(c["G"], geo, np.random.default_rng(c["seed"]), extra=300)
    assert place["shared threads"].shape[0] == 4 * (geo["gb"] // 1024)
    _, ran = _cell(hip_lib, oracle_lib, monkeypatch, name)
    want = {"k_scatter_ac", "k_bucket_accept", "k_bucket_commit", "k_emit_runs", "k_bucket_propose", "k_bucket_prepare"}
    assert want <= ran, (sorted(want - ran), sorted(ran))
    # five replicas, batches grouped by group (the direct back end beside the wide partition)
    _, ran = _cell(hip_lib, oracle_lib, monkeypatch, name, kmax=5, seed=c["seed"] + 1, ordered=True)
    assert {"k_scatter_ac", "k_bucket_accept", "k_bucket_commit"} <= ran, sorted(ran)


@pytest.mark.parametrize("shift", [11, 12])
def test_coordinator_paths_under_wide_buckets(hip_lib, oracle_lib, monkeypatch, shift):
    """The election fuzz (k_bucket_prepare_reply), the request batcher (k_bucket_reqbatch) and accept-reply packing
    (k_bucket_pack_ar) with buckets wider than a workgroup: a tuning switch must not change results."""
    _env(monkeypatch, dict(GPX_BUCKET_SHIFT=shift))
    a = E.fuzz_run(hip_lib, 5, G=2500, steps=40)
    b = E.fuzz_run(oracle_lib, 5, G=2500, steps=40)
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x == y, f"election fuzz entry {i} ({x[0]})"
    for hot in (True, False):
        ra = H.request_batch_run(hip_lib, 3, hot=hot)
        rb = H.request_batch_run(oracle_lib, 3, hot=hot)
        for (la, sa, ba), (lb, sb, bb) in zip(ra, rb):
            assert sa == sb and la == lb and ba == bb
    from tests.test_wire_gpu import test_pack_accept_replies_fuzz
    test_pack_accept_replies_fuzz(hip_lib, oracle_lib, 1)
