"""tests/test_lifetime_gpu.py without a GPU: the same drivers (tests/lifetime_common.py) oracle against oracle, and the
conditions that keep the GPU legs from being vacuous - enough calls per fuzz cell for the wrap to happen at least twice,
an irregular batch next to a regular one at every epoch value, the counters' arithmetic across 2^31 and 2^32, every
ordered pair of front ends as consecutive calls with the route tests/geometry_common.py gives each call."""
import numpy as np
import pytest

from gigapaxos_amd import ORDERED_PROPOSE, ORDERED_REPLY_RUNS
from tests import lifetime_common as L
from tests.geometry_common import CELLS, geometry


@pytest.mark.parametrize("ordered", [False, True], ids=["shuffled", "ordered"])
@pytest.mark.parametrize("name", sorted(CELLS))
def test_every_cell_wraps_the_call_epoch_at_least_twice(oracle_lib, name, ordered):
    """Leg (a): batch calls per cell >= 3 n for every n the GPU leg runs the cell under (16: GPX_FULL_MATRIX), shuffled
    and grouped; of them the ACCEPT, COMMIT and accept-reply calls - whose kernels read the tagged words - >= 3 n too."""
    for wrap in sorted({L.CELL_WRAP.get(name, 5), 3, 16}):
        steps = L.cell_steps(name, wrap)
        _, ca, _ = L.run_cell_counted(oracle_lib, oracle_lib, CELLS[name], ordered, steps=steps)
        assert ca.total >= 3 * wrap and L.wraps(ca.total, wrap) >= 2, (name, wrap, ca.calls)
        readers = ca.calls["accept"] + ca.calls["commit"] + ca.calls["accept_reply"]
        if wrap <= 5:   # (n = 16: the GPU leg counts the LAUNCHES of those kernels, several per call)
            assert readers >= 3 * wrap, (name, wrap, ca.calls)


def test_epoch_arithmetic():
    assert L.epoch_values(9, 5) == [1, 2, 3, 4, 1, 2, 3, 4, 1]
    assert [L.wraps(c, 5) for c in (4, 5, 8, 9, 15)] == [0, 1, 1, 2, 3]
    assert L.wraps(3 * 5, 5) >= 2 and L.wraps(3 * 3, 3) >= 2 and L.wraps(3 * 16, 16) >= 2


@pytest.mark.parametrize("G", [20_000, 70_000])
def test_ordered_script_pairs_irregular_with_regular_at_every_epoch_value(oracle_lib, G):
    """Leg (b): every call of the script draws X.epoch and one_epoch together (an ordered, promised batch each), so call
    i runs at epoch i mod 4 + 1 under n = 5."""
    wrap = 5
    ea, eb = L.make_ordered_pair(oracle_lib, oracle_lib, G, L.MASK_PAC, L.MASK_PAC)
    log = L.run_ordered_script(ea, eb, [L.Population(0, G)], [0] * L.ORDERED_CALLS)
    irr = [x["irregular"] for x in log]
    assert len(log) >= 4 * wrap and L.wraps(len(log), wrap) >= 2
    ir, ri = L.pairing(irr, wrap)
    assert ir == ri == set(range(1, wrap)), (ir, ri)
    # every kind of irregular batch, and a broken promise of each operation behind the first wrap
    assert {x["kind"] for x in log} >= L.IRREGULAR
    late = {x["kind"] for x in log[wrap:]}
    assert {"AX", "CX", "PX"} <= late
    # the work kernels the engine must name (restated dispatch).  20,000 groups with lazy outputs: both one-launch forms,
    # every call draws one_epoch with X.epoch (the pairing above holds for the verdict word too).  70,000 without: check +
    # work kernel for the whole-table batches; the partial ones (a third, a half of the table) fit k_ac_small, which
    # draws no one_epoch - there the pairing is X.epoch's alone
    ks = {L.ordered_kernel(x["op"], x["n"], lazy=G <= 65536) for x in log}
    if G == 20_000:
        assert ks == {"k_ac_pers", "k_propose_pers"}, ks
    else:
        assert {"k_ac_one", "k_propose_one"} <= ks, ks
    L.assert_same_rows(ea, eb, G)


def test_runs_script_pairs_irregular_with_regular(oracle_lib):
    wrap, G = 5, 20_000
    mask = ORDERED_PROPOSE | ORDERED_REPLY_RUNS
    ea, eb = L.make_ordered_pair(oracle_lib, oracle_lib, G, mask, mask, max_batch=3 * G + 64)
    log = L.run_runs_script(ea, eb, G)
    assert len(log) >= 4 * wrap
    ir, ri = L.pairing([x["irregular"] for x in log], wrap)
    assert ir == ri == set(range(1, wrap)), (ir, ri)
    assert max(x["n"] for x in log) <= 65536          # the runs call's one-launch form
    assert [x["kind"] for x in log[wrap:]].count("RX") >= 2


@pytest.mark.parametrize("promised", [False, True])
def test_small_draw_passes_2_32_in_the_middle_of_a_launch(oracle_lib, promised):
    """Leg (c): the chunks k_ac_small draws, added up as the engine adds them."""
    mask = L.MASK_PAC if promised else 0
    pops, schedule, G = L.small_plan()
    ea, eb = L.make_ordered_pair(oracle_lib, oracle_lib, G, mask, mask)
    log = L.run_ordered_script(ea, eb, pops, schedule, promised=promised)
    inc = L.small_increments(log)
    launches = sum(1 for x in inc if x)
    assert launches >= 3 * 5 and max(x["n"] for x in log) == 65536
    before, after, straddle, end = L.crossing(L.SMALL_BASE, inc, 1 << 32)
    assert before >= 5 and after >= 5 and straddle and end > 1 << 32, (before, after, straddle, end)
    # the launch that straddles the boundary has 64 chunks, the boundary falls inside it
    v = L.SMALL_BASE
    for x in inc:
        if x and v < 1 << 32 < v + x:
            assert x == 64 and v + 16 < 1 << 32 < v + 48
        v += x
    # chunks with non-zero totals: commits that execute and ACCEPTs that release runs, in several chunks
    assert any(x["kind"] in ("C", "C3b", "C3c", "AR") and x["n"] > 4 * L.GPX_DCHUNK for x in log)
    L.assert_same_rows(ea, eb, G)


@pytest.mark.parametrize("boundary", [1 << 31, 1 << 32])
def test_arrival_counters_pass_the_boundary(oracle_lib, boundary):
    """Leg (d): gx_arrive's increments (padded grid / 16) of the one-launch calls, added up as xchg_ctl adds them."""
    pops, schedule, G = L.exchange_plan()
    ea, eb = L.make_ordered_pair(oracle_lib, oracle_lib, G, L.MASK_PAC, L.MASK_PAC)
    log = L.run_ordered_script(ea, eb, pops, schedule)
    inc = L.exchange_increments(log)
    before, after, straddle, end = L.crossing(boundary - 5, inc, boundary)
    assert before >= 5 and after >= 5 and straddle and end > boundary, (before, after, straddle, end)
    sizes = {x["n"] for x in log}
    assert min(sizes) <= 2_500 and max(sizes) == 65_000
    ks = {L.ordered_kernel(x["op"], x["n"], lazy=True) for x in log}
    assert ks == {"k_ac_pers", "k_propose_pers", "k_ac_one", "k_propose_one"}, ks
    L.assert_same_rows(ea, eb, G)


def test_increment_restatement():
    assert [L.exchange_increment("accept", n) for n in (1, 2_500, 4_096, 4_097, 13_000, 40_000, 49_152, 49_153, 65_000)] == \
        [1, 1, 1, 2, 4, 10, 12, 0, 0]
    assert [L.exchange_increment("propose", n) for n in (2_500, 32_768, 32_769)] == [1, 8, 0]
    assert [L.small_chunks(n) for n in (1, 1024, 1025, 65536)] == [1, 1, 2, 64]


@pytest.mark.parametrize("seed", [1, 2])
def test_alternation_sequence_has_every_pair_of_front_ends(seed):
    """Leg (g): the driver's own check, and the route geometry_common gives each call at both table sizes."""
    seq = L.alternation_sequence(seed)
    assert len(seq) >= 40
    fes = [L.SHAPES[s] for s in seq]
    assert {(a, b) for a, b in zip(fes, fes[1:])} == {(a, b) for a in L.FRONT_ENDS for b in L.FRONT_ENDS}
    for G in (300_000, (1 << 20) + 1):
        geo = geometry(G, 3)
        rng = np.random.default_rng(seed)
        newest = np.ones(G, np.int32)
        tiles = set()
        for shape in sorted(set(seq)):
            n = L.shape_votes(shape, G, newest, rng)[0].shape[0]
            fe, want, _ = L.shape_route(shape, geo, n)
            assert fe == L.SHAPES[shape], (G, shape, n, fe)
            if shape in ("few tiles", "many tiles"):
                from tests.geometry_common import ar_route
                tiles.add(ar_route(geo, n)[1])
        assert tiles == {4096, 12288}, (G, tiles)


def test_alternation_oracle_against_oracle(oracle_lib):
    G, seed = 300_000, 1
    assert geometry(G, 3)["nbk"] == 586
    seq = L.alternation_sequence(seed)
    ea, eb = L.make_alternation_pair(oracle_lib, oracle_lib, G, seed)
    log = L.run_alternation(L.HostAsDev(ea), eb, G, seq, seed)
    assert len(log) == len(seq) and sum(x["decided"] for x in log) > 2 * G
    assert sum(1 for x in log if x["decided"]) > len(log) // 2
