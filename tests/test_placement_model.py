"""CPU checks of tests/placement_common.py, oracle against oracle: the arenas' geometry, the same placements over numpy
bytes through the oracle's host pointers (guards and poison checked as on the GPU), the cap of test_placement_gpu.py's
cells - every (entry point, placement) pair in every cell, counted with the cells' own seeds: the fuzz draws the same
stream whichever library answers - and the liveness of the poison: handed to the oracle as records, the band behind a
call's columns changes an output column, a counter or the state of the groups it names, and the band in front
changes the answer for the group of record 0.  A poison that changes nothing fails here."""
import numpy as np
import pytest

from gigapaxos_amd import S_UNORDERED
from tests import placement_common as PC
from tests.geometry_common import CELLS, run_cell

# the oracle knows no kernels: `one` and `pers`, `tiles` and `partition` are the same calls to it
MODEL_CASES = [(k, n) for k in ("order", "one", "small", "runs", "tiles") for n in PC.CASES[k][3]]


def _col(name, width, n, out, seed=0):
    if out:
        return PC.Column(name, width, n, True)
    dt = np.int32 if width == 4 else np.uint8
    mk = lambda lo: (np.arange(lo, lo + n if lo == 1000 else lo + PC.P) % 251).astype(dt)  # noqa: E731
    return PC.Column(name, width, n, False, (np.arange(1000, 1000 + n) % 251).astype(dt), mk(1), mk(500))


@pytest.mark.parametrize("placement", PC.NAMES)
@pytest.mark.parametrize("n", [1, 7, 33])
def test_arena_geometry(placement, n):
    """Every column at the offset its placement names, 4 KiB of guard on both sides (under `packed`: around the run,
    the columns back to back), the poison against the column, sentinels around the outputs."""
    cols = [_col("gidx", 4, n, False), _col("slot", 4, n, False), _col("a_flags", 1, n, False),
            _col("r_bnum", 4, n, True), _col("n_runs", 4, 1, True), _col("status", 1, n, True)]
    img = PC.lay_out(placement, cols)
    assert img.shape[0] % 16 == 0
    spans = sorted((c.off, c.off + c.nbytes, c) for c in cols)
    for (a0, a1, a), (b0, b1, b) in zip(spans, spans[1:]):
        assert b0 - a1 >= 2 * PC.GUARD or (placement == "packed" and b0 == a1 and a.out == b.out), (a.name, b.name)
    assert spans[0][0] >= PC.GUARD and img.shape[0] - spans[-1][1] >= PC.GUARD
    for c in cols:
        assert c.off % c.width == 0
        if placement != "packed":
            assert c.off % 16 == PC.offsets_of(placement, c)
        body = img[c.off:c.off + c.nbytes]
        if c.out:
            assert (body == PC.SENTINEL).all()
            lone = placement != "packed"
            if lone:
                assert (img[c.off - PC.GUARD:c.off] == PC.SENTINEL).all()
                assert (img[c.off + c.nbytes:c.off + c.nbytes + PC.GUARD] == PC.SENTINEL).all()
        else:
            assert body.tobytes() == c.body.tobytes()
            if placement != "packed" or c.name == "gidx":
                assert img[c.off - PC.P * c.width:c.off].tobytes() == c.front.tobytes()
            if placement != "packed" or c.name == "a_flags":
                assert img[c.off + c.nbytes:c.off + c.nbytes + PC.P * c.width].tobytes() == c.behind.tobytes()
    assert PC.offsets_of("only-gidx", cols[0]) == 4 and PC.offsets_of("only-gidx", cols[1]) == 0
    # the check itself: a byte changed anywhere outside the outputs' entries is found and named
    after = img.copy()
    PC.verify(img, after, cols, "untouched")
    last = cols[5 if placement == "packed" else 3]   # (packed: behind r_bnum lies the next output's head)
    after[last.off + last.nbytes] ^= 1
    with pytest.raises(AssertionError, match="behind output column " + last.name):
        PC.verify(img, after, cols, "one byte behind an output")
    after = img.copy()
    after[cols[0].off - 1] ^= 1
    with pytest.raises(AssertionError, match="in front of input column gidx"):
        PC.verify(img, after, cols, "one byte in front of an input")


@pytest.mark.parametrize("grouped", [True, False])
def test_poison_shape(grouped):
    rng = np.random.default_rng(3)
    n = 100
    g = rng.integers(50, 90, n).astype(np.int32)
    if grouped:
        g.sort()
    cols = [g] + [rng.integers(0, 9, n).astype(np.int32) for _ in range(4)] + [np.zeros(n, np.uint8)]
    for gmax in (None, 95):
        front, behind = PC.poison("commit", cols, gmax)
        assert behind[0][0] == g[-1] and front[0][-1] == g[0]
        assert all(x.shape[0] == PC.P for x in front + behind)
        if grouped:
            assert (np.diff(np.concatenate([front[0], g, behind[0]])) >= 0).all()
            assert (behind[0][-1] > g[-1]) == (gmax is not None)
        # ... the next slots of a group, never one slot twice
        for band in (front, behind):
            pairs = list(zip(band[0].tolist(), band[3].tolist()))
            assert not grouped or len(set(pairs)) == PC.P
        assert behind[3][0] == cols[3][-1] + 1 and front[3][-1] == cols[3][0] + 1


def _probe(lib, run, op, k, side, gmax=None):
    """The signature of the k-th eligible call of `op` when it is handed its poison; run(wrap) drives engine a."""
    try:
        run(lambda e: PC.Probe(e, op, k, side, gmax))
    except PC.ProbeDone as d:
        return d
    raise AssertionError(f"the driver never made call {k} of {op}")


@pytest.mark.parametrize("name", sorted(CELLS))
def test_cells_cover_every_placement_with_live_poison(oracle_lib, name):
    c = CELLS[name]
    steps = PC.PLACED_STEPS[name]
    _, ef, _ = run_cell(oracle_lib, oracle_lib, c, steps=steps, counted=PC.Recorder)
    counts = PC.cell_counts(ef.log)
    short = {k: v for k, v in counts.items() if v < 1}
    assert not short, (name, steps, short)
    assert all(ef.count[op] >= len(PC.NAMES) for op in PC.OPS), ef.count
    # one call per entry point: the fuzz's records are random (a proposal for a group that another node coordinates is
    # forwarded, an ACCEPT below the ballot or the window refused, whichever array it stands in), so the call that
    # stands for its entry point is the first of its first PROBED eligible calls whose poison the oracle applies
    # In front of a fuzz call the criterion is the whole call's answer (outputs, counters, the state of the groups the
    # band names): whether the group of record 0 itself takes one more record depends on state the driver does not
    # steer.  The directed cases below steer it and hold the band in front to the answer for that group.
    for op in PC.OPS:
        for i, side in ((0, "behind"), (2, "front, whole call")):
            live = []
            for k in range(PC.PROBED):
                d = _probe(oracle_lib, lambda wrap: run_cell(oracle_lib, oracle_lib, c, steps=steps, counted=wrap), op, k, side)
                live.append(d.sig != ef.sigs[(op, k)][i])
                if live[-1]:
                    break
            assert any(live), f"{name}: the poison {side} the first {PC.PROBED} {op} calls changes nothing"


def test_every_pair_three_times_over_the_file():
    """Eleven cells with every pair at least once each (above): at least three times over test_placement_gpu.py."""
    assert len(CELLS) >= 3 and set(PC.PLACED_STEPS) == set(CELLS)


@pytest.mark.parametrize("W", [8, 64])
def test_view_change_entry_points_under_every_placement(oracle_lib, W):
    """gpx_election_begin and gpx_prepare_reply_batch: test_elect_enum_gpu.py's placed legs over numpy bytes through the
    oracle's host pointers - every (entry point, placement) pair occurs, guards and planes checked as on the GPU."""
    from tests import elect_enum_common as EC
    from tests.test_elect_enum_gpu import PLACED_SAMPLE
    counts = {}
    for placement in PC.NAMES:
        def placed(e):
            p = PC.PlacedHostEngine(e)
            p.fixed = placement
            return p
        st = EC.run_enum(oracle_lib, 3, W, 3, "wrap" if W == 64 else "plain", "dev", sample=PLACED_SAMPLE, driver=placed)
        for k, v in PC.elect_counts(st.driver.log).items():
            counts[k] = counts.get(k, 0) + v
    assert set(counts) == {(op, p) for op in PC.ELECT_ENTRY_POINTS for p in PC.NAMES} and all(v >= 1 for v in counts.values()), counts


def test_view_change_planes_and_wide_columns():
    """lay_out_wide: 8-byte columns on 8-byte boundaries under every placement, every column between its guards."""
    n, W, m = 5, 8, 7
    for placement in PC.NAMES:
        cols = [PC.WideColumn("gidx", 4, n, False, np.arange(n, dtype=np.int32), np.zeros(PC.P, np.int32), np.ones(PC.P, np.int32)),
                PC.WideColumn("pv_handle", 8, m, False, np.arange(m, dtype=np.int64), np.zeros(PC.P, np.int64), np.ones(PC.P, np.int64)),
                PC.WideColumn("pv_flags", 1, m, False, np.zeros(m, np.uint8), np.zeros(PC.P, np.uint8), np.ones(PC.P, np.uint8)),
                PC.WideColumn("e_handle", 8, n * W, True), PC.WideColumn("e_slot", 4, n * W, True), PC.WideColumn("status", 1, n, True)]
        img = PC.lay_out_wide(placement, cols)
        spans = sorted((c.off, c.off + c.nbytes, c) for c in cols)
        assert spans[0][0] >= PC.GUARD and img.shape[0] - spans[-1][1] >= PC.GUARD
        for (a0, a1, a), (b0, b1, b) in zip(spans, spans[1:]):
            assert b0 - a1 >= 2 * PC.GUARD or (placement == "packed" and b0 == a1 and a.out == b.out), (placement, a.name, b.name)
        for c in cols:
            assert c.off % c.width == 0
            if c.out:
                assert (img[c.off:c.off + c.nbytes] == PC.SENTINEL).all()
            else:
                assert img[c.off:c.off + c.nbytes].tobytes() == c.body.tobytes()


def test_view_change_poison_is_live(oracle_lib):
    """Handed to the oracle as records, the band behind the record columns changes the state of the group of record
    n - 1; one entry of the band behind the pvalue columns, read by the last record, changes what that group carries."""
    from tests import elect_enum_common as EC
    S0 = EC.BASES["plain"]
    g = np.arange(4, dtype=np.int32)
    acc = np.array([101, 7, 5000, 7], np.int32)
    pvalues = [[(S0, 0, 7, 600 + i, 0)] for i in range(4)]
    off, pv = EC.flatten(pvalues)
    cols = [g, acc, np.full(4, EC.BNUM, np.int32), np.full(4, EC.ME, np.int32), np.full(4, S0, np.int32)]
    front, behind = PC.elect_poison("prepare_reply", cols + [off] + list(pv))

    def dumps(cols_, pvalues_):
        e = EC.make_engine(oracle_lib, 3, 8, 4, S0, 64)
        assert (e.election_begin(g, np.full(4, EC.BNUM, np.int32)) == 0).all()
        e.prepare_reply(*cols_, pvalues_)
        out = [e.dump(int(x)).tolist() for x in g]
        e.close()
        return out
    plain = dumps(cols, pvalues)
    ext = [np.concatenate([c, b]) for c, b in zip(cols, behind[:5])]
    assert dumps(ext, pvalues + [[] for _ in range(PC.P)])[3] != plain[3]
    extra = tuple(int(behind[6 + i][0]) for i in range(5))
    assert extra[1] == 1 and extra[4] & 1 and extra[3] != 600
    assert dumps(cols, pvalues[:3] + [pvalues[3] + [extra]])[3] != plain[3]
    pre = [np.concatenate([f, c]) for c, f in zip(cols, front[:5])]
    assert dumps(pre, [[] for _ in range(PC.P)] + pvalues)[0] != plain[0]


@pytest.mark.parametrize("kind,n", MODEL_CASES)
def test_directed_cases_with_live_poison(oracle_lib, kind, n):
    """Every case of test_placement_gpu.py's tails, the oracle through placed numpy columns against the oracle; then
    every data call of the case once more with its poison handed over as records."""
    G, mask = PC.CASES[kind][1], PC.CASES[kind][2]
    sigs = None
    for placement in ("all+4", "packed"):
        ea, eb = PC.case_engine(oracle_lib, kind), PC.case_engine(oracle_lib, kind)
        ra = PC.Recorder(ea, first_only=False)
        ra.fixed, ra.gmax = placement, G - 1
        PC.drive_case(kind, n, ra, eb)
        sigs = ra.sigs
        ea.close(), eb.close()
    data_ops = PC.CASES[kind][4]
    assert {op for op, _ in sigs} >= set(data_ops)
    for (op, k), base in sigs.items():
        if op not in data_ops:
            continue
        for i, side in enumerate(("behind", "front")):
            def run(wrap):
                ea, eb = PC.case_engine(oracle_lib, kind), PC.case_engine(oracle_lib, kind)
                PC.drive_case(kind, n, wrap(ea), eb)
            d = _probe(oracle_lib, run, op, k, side, G - 1)
            if op == "propose" and mask & 1 and side == "behind":
                # the strict promise of proposal batches (no group twice): the first record behind names the group of
                # record n - 1 and is refused with everything after it - a call that ran on would answer for it all the
                # same, and a successor read without its guard merges record n - 1 into that run
                assert (d.tail_status == S_UNORDERED).all() and d.sig == base[i]
                continue
            assert d.sig != base[i], f"{kind} n={n}: the poison {side} {op} call {k} changes nothing"
