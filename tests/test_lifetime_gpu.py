"""Long-lived engines: what one call leaves behind for a later one.

The kernels do not clear their scratch between calls; they tag it with a per-call epoch (X.epoch, one_epoch,
small_epoch, w_epoch) and compare tags, and the arrival / ticket counters (gx_arrive, small_draw) only count up.  The
wrap branches of the epochs and the counters' 2^31 / 2^32 boundaries are days of calls away; GPX_TEST_EPOCH_WRAP and
GPX_TEST_COUNTER_BASE bring them into a test.  Engine against oracle, bit for bit, through the C-ABI; the
drivers are those of tests/lifetime_common.py, which tests/test_lifetime_model.py runs oracle against oracle.

  a  every back end's fuzz cell (geometry_common.CELLS, grouped batches) across the call epoch's wrap
  b  ordered batches - one-launch form, check + work kernel, lazy outputs, gpx_compact_last_dev after every call -
     with an irregular batch next to a regular one at every epoch value; the runs call's one-launch form
  c  k_ac_small, both instantiations, across small_epoch's wrap and with small_draw passing 2^32 inside a launch
  d  grid_exchange's arrival counters across 2^31 and 2^32; eight engines on their own threads under the wrap
  e  gpx_wire_decode across w_epoch's wrap, both tilings
  f  four asynchronous calls in flight across the wrap (the wrap synchronises ONE stream; copies sit on others)
  g  accept-reply calls of every shape and front end alternating on one engine

Every leg reads gpx_profile_read and asserts that the kernels which consume the counter under test ran at least 3 n
times (n = the leg's GPX_TEST_EPOCH_WRAP: the wrap branch ran at least twice) or, for the cumulative counters, that the
increments - added up as the engine adds them - passed the boundary with five launches on either side."""
import os
import threading

import numpy as np
import pytest

from gigapaxos_amd import (Engine, hri_create, streams, S_OK, LAZY_OUTPUTS, ORDERED_PROPOSE, ORDERED_REPLY_RUNS)
from gigapaxos_amd._abi import GpxError
from tests import lifetime_common as L
from tests.geometry_common import CELLS, geometry, ac_kernels
from tests.parity_common import make_pair

pytestmark = pytest.mark.gpu
FULL = os.environ.get("GPX_FULL_MATRIX") == "1"
BACKEND_SWITCHES = ("GPX_AR_TILES", "GPX_TRY_RUNS", "GPX_SAR_MAX_N", "GPX_BUCKET_SHIFT", "GPX_TILE_T", "GPX_TILE_NT",
                    "GPX_XCHG_SLOTS", "GPX_WD_TILE") + L.SWITCHES


@pytest.fixture(autouse=True)
def _clean_switches(monkeypatch):
    for v in BACKEND_SWITCHES:
        monkeypatch.delenv(v, raising=False)


def _wrap(monkeypatch, hip_lib, n):
    """GPX_TEST_EPOCH_WRAP=n for the engines created from here on - after showing that the library reads that name."""
    L.assert_switch_is_read(monkeypatch, hip_lib, "GPX_TEST_EPOCH_WRAP")
    monkeypatch.setenv("GPX_TEST_EPOCH_WRAP", str(n))


def _base(monkeypatch, hip_lib, v):
    L.assert_switch_is_read(monkeypatch, hip_lib, "GPX_TEST_COUNTER_BASE")
    monkeypatch.setenv("GPX_TEST_COUNTER_BASE", str(v))


def test_bad_switch_values_are_refused(hip_lib, monkeypatch):
    for name, bad in (("GPX_TEST_EPOCH_WRAP", ("1", "0", "-4", "5x", "")), ("GPX_TEST_COUNTER_BASE", ("-1", "4294967296", "x"))):
        for v in bad:
            monkeypatch.setenv(name, v)
            with pytest.raises(GpxError):
                Engine(hip_lib, 100, 64, kmax=3, window=8, max_batch=1024)
        monkeypatch.delenv(name)
    Engine(hip_lib, 100, 64, kmax=3, window=8, max_batch=1024).close()


# ---- a ---------------------------------------------------------------------------------------------------------------------
def _cells():
    if not FULL:
        cells = [(name, n) for name, n in L.CELL_WRAP.items()]
    else:
        cells = [(name, n) for name in CELLS for n in sorted({L.CELL_WRAP.get(name, 5), 3, 16})]
    return [(name, n, ordered) for name, n in cells for ordered in (False, True)]


@pytest.mark.parametrize("name,wrap,ordered", _cells(),
                         ids=lambda v: {False: "shuffled", True: "ordered"}.get(v, str(v)) if isinstance(v, bool) else str(v))
def test_every_back_end_across_the_call_epochs_wrap(hip_lib, oracle_lib, monkeypatch, name, wrap, ordered):
    """The cell's fuzz, shuffled (the cell's own back end for every batch) and with batches grouped by group (the direct
    back end beside it; one batch in eight carries an index out of range and takes the partition), the call epoch coming
    round every wrap - 1 calls: *X.unsorted, rec_tag, D.mark and A.ref[3] of an earlier cycle meet their epoch value
    again all the time."""
    c = CELLS[name]
    _wrap(monkeypatch, hip_lib, wrap)
    for k, v in c["env"].items():
        monkeypatch.setenv(k, str(v))
    seen, ca, prof = L.run_cell_counted(hip_lib, oracle_lib, c, ordered, steps=L.cell_steps(name, wrap))
    assert ca.total >= 3 * wrap and L.wraps(ca.total, wrap) >= 2, ca.calls
    readers = sum(prof.get(k, 0) for k in L.EPOCH_READERS)
    assert readers >= 3 * wrap, prof
    assert all(seen[op] for op in ("propose", "accept", "accept_reply", "commit", "prepare")), seen
    ran = set(prof)
    geo = geometry(c["G"], c["kmax"], c.get("shift"))
    # the kernels geometry_common predicts for the cell's ACCEPT / COMMIT batches (both back ends are launched, the
    # device picks) and test_backends_gpu.py's for its accept-reply calls
    for op, n in ca.sizes:
        if op in ("accept", "commit"):
            assert ac_kernels(geo, n, op) <= ran, (op, n, sorted(ac_kernels(geo, n, op) - ran))
    if name.startswith("partition-"):
        assert {"k_hist", "k_scatter_ar16", "k_bucket_ar16", "k_emit_dec16"} <= ran, sorted(ran)
        assert "k_ar_tiny" not in ran and "k_scatter_tiles" not in ran, sorted(ran)
    elif name.startswith("tiles-"):
        assert {"k_scatter_tiles", "k_emit_dec16"} <= ran and "k_ar_tiny" not in ran and "k_scatter_ar16" not in ran, sorted(ran)
    elif name.startswith("runs-"):
        assert any(k.startswith(("k_runs_check", "k_ar_runs")) for k in ran) and "k_ar_tiny" not in ran, sorted(ran)
    elif name.startswith("big-"):
        assert {"k_order_check", "k_scatter_ac16", "k_bucket_accept16", "k_bucket_commit16", "k_emit_runs16"} <= ran, sorted(ran)
        assert "k_ac_small" not in ran, sorted(ran)
    else:
        want = {"k_scatter_ac", "k_bucket_accept", "k_bucket_commit"}
        if not ordered:
            want |= {"k_emit_runs", "k_bucket_propose", "k_bucket_prepare"}
        assert want <= ran, (sorted(want - ran), sorted(ran))


# ---- b ---------------------------------------------------------------------------------------------------------------------
ORDERED_CASES = [pytest.param(20_000, True, True, id="one launch, lazy outputs", marks=pytest.mark.gpu_fast),
                 pytest.param(20_000, True, False, id="check + work kernel, lazy outputs"),
                 pytest.param(70_000, False, True, id="check + work kernel, compacted at once")]


@pytest.mark.parametrize("G,lazy,exchange", ORDERED_CASES)
def test_ordered_batches_irregular_next_to_regular_across_the_wrap(hip_lib, oracle_lib, monkeypatch, G, lazy, exchange):
    """lifetime_common's script of ordered PROPOSE / ACCEPT / COMMIT batches under the promises, n = 5: call i runs at
    call epoch i mod 4 + 1 and - where every call draws a verdict epoch, i.e. with lazy outputs - at the same one_epoch.
    Blocks of four irregular and four regular batches: each epoch value sees a batch that writes D.mark, tags, *X.unsorted
    or the verdict word and, four calls later, one that must not find them - and the other way round.
    gpx_compact_last_dev follows every call.  A batch that breaks its promise behind a wrap is refused from its first
    violation on (run_ordered_script asserts it on the oracle's answer, which the engine's must equal)."""
    wrap = 5
    _wrap(monkeypatch, hip_lib, wrap)
    if not exchange:
        monkeypatch.setenv("GPX_XCHG_SLOTS", "0")
    eh, eo = L.make_ordered_pair(hip_lib, oracle_lib, G, L.MASK_PAC | (LAZY_OUTPUTS if lazy else 0), L.MASK_PAC)
    dev = L.DevEngine(eh)
    log = L.run_ordered_script(dev, eo, [L.Population(0, G)], [0] * L.ORDERED_CALLS)
    ir, ri = L.pairing([x["irregular"] for x in log], wrap)
    assert ir == ri == set(range(1, wrap)), (ir, ri)
    for i, (x, ks) in enumerate(zip(log, dev.kernels)):
        want = L.ordered_kernel(x["op"], x["n"], lazy, one_launch=exchange)
        assert want in ks, (i, x, sorted(ks))
        if want.endswith("_one"):
            assert "k_one_check" in ks, (i, x, sorted(ks))
        if lazy and x["op"] != "propose":   # the count word as the call left it: parked outputs iff the batch is irregular
            assert (x["raw"] < 0) == x["irregular"], (i, x)
    drew = sum(dev.launches.get(k, 0) for k in ("k_ac_pers", "k_propose_pers", "k_one_check"))
    assert drew >= 3 * wrap, dev.launches                       # one_epoch
    assert len(log) >= 4 * wrap and L.wraps(len(log), wrap) >= 2  # X.epoch: every call
    L.assert_same_rows(eh, eo, G)
    eh.close(), eo.close()


@pytest.mark.parametrize("exchange", [True, False])
def test_reply_runs_calls_across_the_wrap(hip_lib, oracle_lib, monkeypatch, exchange):
    """The runs call under ORDERED_REPLY_RUNS | LAZY_OUTPUTS (60,000 votes: its one-launch form, k_ar_runs<.., SMALL>,
    draws from one_epoch like the proposals between): regular rounds, rounds with lost votes, votes that come again, and
    batches that break the promise - refused whole, behind a wrap as before it."""
    wrap, G = 5, 20_000
    _wrap(monkeypatch, hip_lib, wrap)
    if not exchange:
        monkeypatch.setenv("GPX_XCHG_SLOTS", "0")
    mask = ORDERED_PROPOSE | ORDERED_REPLY_RUNS
    eh, eo = L.make_ordered_pair(hip_lib, oracle_lib, G, mask | LAZY_OUTPUTS, mask, max_batch=3 * G + 64)
    dev = L.DevEngine(eh)
    log = L.run_runs_script(dev, eo, G)
    ir, ri = L.pairing([x["irregular"] for x in log], wrap)
    assert ir == ri == set(range(1, wrap)), (ir, ri)
    for i, (x, ks) in enumerate(zip(log, dev.kernels)):
        if x["kind"] == "P":
            assert ("k_propose_pers" if exchange else "k_propose_one") in ks, (i, sorted(ks))
        else:
            assert ("k_ar_runs_pers" if exchange else "k_ar_runs") in ks, (i, sorted(ks))
            assert (x["raw"] < 0) == x["irregular"] or x["kind"] == "RX", (i, x)
    drew = sum(dev.launches.get(k, 0) for k in ("k_ar_runs_pers", "k_propose_pers", "k_one_check", "k_runs_check"))
    assert drew >= 3 * wrap, dev.launches
    L.assert_same_rows(eh, eo, G)
    eh.close(), eo.close()


# ---- c ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("promised", [False, True])
def test_small_fused_calls_across_small_epochs_wrap_and_2_32_chunks(hip_lib, oracle_lib, monkeypatch, promised):
    """k_ac_small<false> (ACCEPT) and <true> (COMMIT), unpromised (a batch out of order goes to the partition launched
    behind) and promised (refused from the violation on), without lazy outputs: a workgroup takes the chunk it DRAWS
    (draw - draw_base, unsigned) and waits for the tickets of the chunks before it to carry this launch's epoch.
    small_draw starts at 2^32 - 37: five launches of one chunk, then a launch of 64 chunks draws 2^32 - 32 .. 2^32 + 31."""
    wrap = 5
    _wrap(monkeypatch, hip_lib, wrap)
    _base(monkeypatch, hip_lib, L.SMALL_BASE)
    mask = L.MASK_PAC if promised else 0
    pops, schedule, G = L.small_plan()
    eh, eo = L.make_ordered_pair(hip_lib, oracle_lib, G, mask, mask)
    dev = L.DevEngine(eh)
    log = L.run_ordered_script(dev, eo, pops, schedule, promised=promised)
    inc = L.small_increments(log)
    for i, (x, ks, d) in enumerate(zip(log, dev.kernels, inc)):
        assert ("k_ac_small" in ks) == (d > 0), (i, x, sorted(ks))
    launches = sum(1 for d in inc if d)
    assert dev.launches.get("k_ac_small", 0) == launches >= 3 * wrap, dev.launches
    before, after, straddle, end = L.crossing(L.SMALL_BASE, inc, 1 << 32)
    assert before >= 5 and after >= 5 and straddle and end > 1 << 32, (before, after, straddle, end)
    eh.sync()
    L.assert_same_rows(eh, eo, G)
    eh.close(), eo.close()


# ---- d ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("boundary", [1 << 31, 1 << 32], ids=["2^31", "2^32"])
def test_arrival_counters_across_the_boundary(hip_lib, oracle_lib, monkeypatch, boundary):
    """One engine, ordered batches of 2,500 .. 65,000 records with lazy outputs: k_ac_pers / k_propose_pers meet at the
    sixteen arrival counters, whose target the host counts up (gx_arrive) and which the pollers compare by signed
    difference.  Counters and target start five increments below the boundary and pass it inside the fifth one-launch
    call.  A poller that gave up would surface as GPX_EDEVICE from the call or from gpx_engine_sync."""
    _base(monkeypatch, hip_lib, (boundary - 5) & 0xffffffff)
    pops, schedule, G = L.exchange_plan()
    eh, eo = L.make_ordered_pair(hip_lib, oracle_lib, G, L.MASK_PAC | LAZY_OUTPUTS, L.MASK_PAC)
    dev = L.DevEngine(eh)
    log = L.run_ordered_script(dev, eo, pops, schedule)
    inc = L.exchange_increments(log)
    for i, (x, ks, d) in enumerate(zip(log, dev.kernels, inc)):
        assert L.ordered_kernel(x["op"], x["n"], True) in ks, (i, x, sorted(ks))
        assert bool(ks & {"k_ac_pers", "k_propose_pers"}) == (d > 0), (i, x, sorted(ks))
    pers = dev.launches.get("k_ac_pers", 0) + dev.launches.get("k_propose_pers", 0)
    assert pers == sum(1 for d in inc if d) and dev.launches.get("k_ac_pers", 0) and dev.launches.get("k_propose_pers", 0)
    before, after, straddle, end = L.crossing(boundary - 5, inc, boundary)
    assert before >= 5 and after >= 5 and straddle and end > boundary, (before, after, straddle, end)
    eh.sync()   # GPX_OK: nobody gave up
    L.assert_same_rows(eh, eo, G)
    eh.close(), eo.close()


def test_eight_engines_on_their_own_threads_across_the_wrap(hip_lib, oracle_lib, monkeypatch):
    """test_many_engines_gpu.py's eight engines, four rounds each (16 batch calls per engine), every engine's epochs
    wrapping at 5: each has its own counters, they share the device."""
    from tests.test_many_engines_gpu import _drive
    wrap, rounds = 5, 4
    _wrap(monkeypatch, hip_lib, wrap)
    pe = L.ProfiledEngines(monkeypatch, hip_lib)
    sizes = [13_000, 2_500, 40_000, 65_000, 7_000, 30_000, 5_000, 17_000]
    out = [None] * len(sizes)
    start = threading.Barrier(len(sizes))

    def run(i):
        start.wait()
        _drive(hip_lib, oracle_lib, sizes[i], rounds, 200 + i, out, i)
    holders = [Engine(hip_lib, 100, 64, kmax=3, window=8, max_batch=1024) for _ in sizes]
    threads = [threading.Thread(target=run, args=(i,), daemon=True) for i in range(len(sizes))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=240)
    alive = [i for i, t in enumerate(threads) if t.is_alive()]
    assert not alive, f"engines {alive} did not finish"
    for h in holders:
        h.close()
    assert all(o and o[0] == "ok" for o in out), out
    assert len(pe.profiles) == len(sizes) and min(pe.calls()) >= 3 * wrap, pe.profiles   # per engine


# ---- e ---------------------------------------------------------------------------------------------------------------------
# (a build that forgets to clear the look-back words at the wrap fails [256-3] only - profiles/r10_lifetime_tests.txt: with
# 512-frame tiles or n = 5 the tile in front has always written before its word is read; those cases show that the wrap
# changes no answer, not that the clear is needed)
WIRE_CASES = [(512, 5), (256, 3), (512, 3), (256, 5)]


@pytest.mark.parametrize("tile,wrap", WIRE_CASES)
def test_wire_decode_across_w_epochs_wrap(hip_lib, oracle_lib, monkeypatch, tile, wrap):
    """4 n consecutive gpx_wire_decode calls on one engine, bursts of 2,400 frames and more (several tiles: the look-back
    words `epoch << 40 | state << 38 | count` of the tiles before are read): damage 0, damage 0.3, and bursts of heavy
    and light tiles."""
    from tests.wire_common import make_wire_pair, random_frames, assert_same_decode
    _wrap(monkeypatch, hip_lib, wrap)
    monkeypatch.setenv("GPX_WD_TILE", str(tile))
    rng = np.random.default_rng(tile + wrap)
    ((eh, wh), (eo, wo)), names = make_wire_pair(hip_lib, oracle_lib, 1500, 3, rng)
    # four bursts, taken in an order of seven (not a divisor of the epochs' cycle: the words an epoch value finds are another burst's): damage 0,
    # damage 0.3, and heavy and light tiles in turn, where a light tile looks back before the tile in front has written
    bursts = [random_frames(names, 2400, rng, 0.0), random_frames(names, 2400, rng, 0.3),
              L.skewed_frames(names, tile, 8, rng, 1), L.skewed_frames(names, tile, 8, rng, 2)]
    want = [wo.decode(b) for b in bursts]
    assert 2400 > 4 * tile and want[2].counts["n_votes"] > 8 * tile and want[2].counts != want[3].counts
    order = [0, 2, 1, 3, 2, 0, 3]   # seven: coprime to the cycles of n = 3 and n = 5
    eh.profile(2)
    for i in range(4 * wrap):
        b = order[i % len(order)]
        assert_same_decode(wh.decode(bursts[b]), want[b], f"call {i} (burst {b})")
    prof = eh.profile_read()
    assert prof["k_wire_decode1"][0] >= 4 * wrap >= 3 * wrap, prof
    eh.close(), eo.close()


# ---- f ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,pin", [(3000, False), (300_000, False), (300_000, True)])
def test_four_asynchronous_calls_in_flight_across_the_wrap(hip_lib, oracle_lib, monkeypatch, G, pin):
    """test_async_rounds_match_oracle's shape (proposal, votes, ACCEPTs and commits in flight together, five rounds =
    twenty calls, n = 5): begin_front's wrap synchronises the engine's stream and clears words with blocking memsets
    while copies of the other calls are queued on the copy-in and copy-out streams.  pin: registered buffers."""
    wrap, k = 5, 3
    _wrap(monkeypatch, hip_lib, wrap)
    members = list(range(100, 100 + k))
    eh, eo = make_pair(hip_lib, oracle_lib, 100, G, k, 8, max_batch=G * k + G * k // 40 + 4096)
    mem = np.tile(np.array(members, np.int32), (G, 1))
    for e in (eh, eo):
        assert (e.create_groups(np.arange(G), mem, k, hri_create(G, k, 100)) == S_OK).all()
    g = np.arange(G, dtype=np.int32)
    eh.profile(2)
    calls = 0
    for r in range(5):
        po = eo.propose(g)
        cols = streams.vote_round(G, members, r, 100, config_id=4, mix=(r == 3))
        if pin:
            eh.host_register(g, *cols)
        tp = eh.propose_async(g, pin_outputs=pin)
        tv = eh.accept_reply_async(*cols, pin_outputs=pin)
        do = eo.accept_reply(*cols)
        ta = eh.accept_async(g, po[1], po[2], po[0], po[3])
        tc = eh.commit_async(do.gidx, do.bnum, do.bcoord, do.slot, do.median_cp, np.full(do.gidx.shape[0], 1, np.uint8))
        calls += 4
        for x, y in zip(tp.wait(), po):
            assert (x == y).all(), f"round {r} proposals"
        dh = tv.wait()
        assert dh.as_tuple_array().shape == do.as_tuple_array().shape and (dh.as_tuple_array() == do.as_tuple_array()).all()
        assert (dh.status == do.status).all(), f"round {r} votes"
        (ra, xa), (rb, xb) = ta.wait(), eo.accept(g, po[1], po[2], po[0], po[3])
        assert all((x == y).all() for x, y in zip(ra, rb)) and (xa.as_tuple_array() == xb.as_tuple_array()).all()
        (sa, ca), (sb, cb) = tc.wait(), eo.commit(do.gidx, do.bnum, do.bcoord, do.slot, do.median_cp,
                                                   np.full(do.gidx.shape[0], 1, np.uint8))
        assert (sa == sb).all() and (ca.as_tuple_array() == cb.as_tuple_array()).all(), f"round {r} commits"
        if pin:
            eh.host_unregister(g, *cols)
    prof = {k_: v[0] for k_, v in eh.profile_read().items()}
    assert calls >= 4 * wrap and sum(prof.get(k_, 0) for k_ in L.EPOCH_READERS) >= 3 * wrap, prof
    assert eh.snapshot(g)[0].tobytes() == eo.snapshot(g)[0].tobytes()
    assert eh.counters() == eo.counters()
    eh.close(), eo.close()


def test_packed_votes_in_flight_across_the_wrap(hip_lib, oracle_lib, monkeypatch):
    """gpx_accept_reply_packed_async, once: test_packed_gpu.py's rounds under n = 5."""
    from tests.test_packed_gpu import test_packed_rounds_match_oracle
    wrap = 5
    _wrap(monkeypatch, hip_lib, wrap)
    pe = L.ProfiledEngines(monkeypatch, hip_lib)
    test_packed_rounds_match_oracle(hip_lib, oracle_lib, 3000, 3)
    assert len(pe.profiles) == 1 and pe.calls()[0] >= 3 * wrap, pe.profiles


# ---- g ---------------------------------------------------------------------------------------------------------------------
ALT_CASES = [(300_000, None), (300_000, 7), ((1 << 20) + 1, None), ((1 << 20) + 1, 7)]


@pytest.mark.parametrize("G,wrap", ALT_CASES)
def test_front_ends_alternate_on_one_engine(hip_lib, oracle_lib, monkeypatch, G, wrap):
    """At least 40 accept-reply calls of eleven shapes on ONE engine, half of whose groups are out of lock-step - tiny,
    narrow / wide tiles of 4,096 and 12,288 votes, the partition (unaligned device columns), the acceptors' runs and a
    shuffled call under GPX_TRY_REPLY_RUNS (set and cleared at run time), no status column, a lost acceptor, the
    adversarial mix - which all share the tile area, o_rec, rec_tag, chunk_cnt, runs_info and the learnt in-place
    ratio.  The first 17 calls walk through all 16 ordered pairs of front ends with nothing in between; proposals,
    ACCEPTs and COMMITs come between the later ones.  Every call asserts the kernels geometry_common predicts for it."""
    seed = 1
    seq = L.alternation_sequence(seed)
    geo = geometry(G, 3)
    if wrap:
        _wrap(monkeypatch, hip_lib, wrap)
    eh, eo = L.make_alternation_pair(hip_lib, oracle_lib, G, seed)
    dev = L.DevEngine(eh)
    routes = []

    def check(c, shape, n, ks):
        fe, want, never = L.shape_route(shape, geo, n)
        assert fe == L.SHAPES[shape] and want <= ks and not (never & ks), (c, shape, n, sorted(ks))
        if shape in ("runs", "shuffled hint"):
            assert any(k.startswith("k_ar_runs") for k in ks), (c, shape, sorted(ks))
        routes.append(fe)
    log = L.run_alternation(dev, eo, G, seq, seed, check=check)
    assert {(a, b) for a, b in zip(routes[:17], routes[1:17])} == {(a, b) for a in L.FRONT_ENDS for b in L.FRONT_ENDS}
    assert len(log) >= 40 and sum(x["decided"] for x in log) > G
    placed, compacted = eh.path_counters()
    print("in place / compacted:", placed, compacted)
    assert compacted, (placed, compacted)   # a prediction of the in-place form missed: the learnt ratio moved between calls
    if wrap:
        assert len(log) >= 3 * wrap
    eh.close(), eo.close()


def test_in_place_path_counters_across_the_wrap(hip_lib, oracle_lib, monkeypatch):
    """A.ref[3] holds the epoch of the last call some bucket of which missed its predicted span.  test_inplace_gpu.py's
    rounds under n = 3 (epochs 1, 2, 1, 2, ..: every accept-reply call runs at epoch 2): the call after a compacted one
    must be counted in place again - begin_front's wrap clears the word with the other tagged ones."""
    from tests.test_inplace_gpu import test_steady_state_in_place_and_the_ratio_is_learnt
    wrap = 3
    _wrap(monkeypatch, hip_lib, wrap)
    pe = L.ProfiledEngines(monkeypatch, hip_lib)
    test_steady_state_in_place_and_the_ratio_is_learnt(hip_lib, oracle_lib, 250_123, 3)
    assert len(pe.profiles) == 1 and pe.profiles[0].get("k_emit_dec16", 0) >= 2 * wrap, pe.profiles   # its accept-reply calls
    assert pe.calls()[0] >= 3 * wrap, pe.profiles
