"""The step's once-touched streams marked non-temporal (GPX_NT_STREAMS, gigapaxos_amd/csrc/gpx_kernels.hip.h; DESIGN.md
3.3): the vote columns k_scatter_tiles reads and its status prefill, the output columns of k_propose_one /
k_propose_pers, the in-place decision columns and the staging of the per-bucket kernel.  A cache policy changes no
result: every site is driven at the smallest shape that reaches it and compared with the oracle bit for bit - full and
partly filled tiles, a vote count that is no multiple of 4, a status column that is misaligned or absent, every
instantiation of the scatter kernel, staging that k_emit_dec16 reads back, refused and unordered proposals."""
import numpy as np
import pytest

from gigapaxos_amd import hri_create, streams, S_OK, S_UNORDERED, S_WINDOW, ORDERED_PROPOSE
from tests.parity_common import make_pair
from tests.test_fullsize_gpu import _same

pytestmark = pytest.mark.gpu
MEMBERS = [100, 101, 102]
_rounds = {}


def _votes(G, r):
    """Round r of the shuffled config #3 stream for G groups: generated once, shared, never modified."""
    if (G, r) not in _rounds:
        cols = streams.vote_round(G, MEMBERS, r, 100, config_id=3, mix=False)
        for c in cols:
            c.setflags(write=False)
        _rounds[(G, r)] = cols
    return _rounds[(G, r)]


def _pair(hip_lib, oracle_lib, G, window=8):
    eh, eo = make_pair(hip_lib, oracle_lib, 100, G, 3, window, max_batch=3 * G + 4096)
    mem = np.tile(np.array(MEMBERS, np.int32), (G, 1))
    for e in (eh, eo):
        assert (e.create_groups(np.arange(G), mem, 3, hri_create(G, 3, 100)) == S_OK).all()
    return eh, eo


def _propose_both(eh, eo, g, what="propose"):
    ra, rb = eh.propose(g), eo.propose(g)
    for x, y, nm in zip(ra, rb, ("slot", "bnum", "bcoord", "median", "status")):
        assert x.tolist() == y.tolist(), f"{what}: {nm}"
    return ra


@pytest.mark.parametrize("n_drop,status", [(0, "aligned"), (1, "aligned"), (1, "misaligned"), (1, "none")])
def test_tiled_front_end_tail_and_status_forms(hip_lib, oracle_lib, n_drop, status):
    """2,048 groups x 3 = 6,144 votes: above k_ar_tiny's bound, two tiles of 4,096 of which the second is half filled (the
    loads and the prefill that test every entry against n).  n_drop = 1: 6,143 votes, no multiple of 4 - the last vector
    of the batch is cut.  A status column off a 4-byte boundary sends every tile through the byte-wise prefill; without
    one the prefill is skipped.  Two rounds through the device entry point."""
    import torch
    G = 2048
    eh, eo = _pair(hip_lib, oracle_lib, G)
    g = np.arange(G, dtype=np.int32)
    for r in range(2):
        _propose_both(eh, eo, g)
        cols = [c[:c.shape[0] - n_drop].copy() for c in _votes(G, r)]
        n = cols[0].shape[0]
        assert n == 3 * G - n_drop and n > 4096 and (n % 4 != 0) == bool(n_drop)
        dc = [torch.from_numpy(c).cuda() for c in cols]
        d = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(5)] + [torch.zeros(n, dtype=torch.uint8, device="cuda")]
        no = torch.zeros(1, dtype=torch.int32, device="cuda")
        st_buf = torch.full((n + 16,), 0xEE, dtype=torch.uint8, device="cuda")
        off = {"aligned": 0, "misaligned": 1, "none": 0}[status]
        st_ptr = 0 if status == "none" else st_buf.data_ptr() + off
        assert st_buf.data_ptr() % 16 == 0
        torch.cuda.synchronize()
        eh.profile(2)
        eh.call_dev("accept_reply_batch", n, *[t.data_ptr() for t in dc], *[t.data_ptr() for t in d], no.data_ptr(), st_ptr)
        eh.sync()
        assert "k_scatter_tiles" in eh.profile_read()
        eh.profile(0)
        do = eo.accept_reply(*cols)
        m = int(no.item())
        got = np.stack([t[:m].cpu().numpy().astype(np.int32) for t in d], axis=1)
        assert got.shape == do.as_tuple_array().shape and (got == do.as_tuple_array()).all(), f"round {r}"
        sb = st_buf.cpu().numpy()
        if status == "none":
            assert (sb == 0xEE).all()
        else:
            assert (sb[off:off + n] == do.status).all(), f"round {r}: per-vote status"
            assert (sb[:off] == 0xEE).all() and (sb[off + n:] == 0xEE).all(), "a status store outside the column"
    assert eh.snapshot(g)[0].tobytes() == eo.snapshot(g)[0].tobytes()
    assert eh.counters() == eo.counters()
    eh.close(), eo.close()


@pytest.mark.parametrize("T,NT", [(4096, 512), (8192, 512), (4096, 1024), (8192, 1024), (12288, 1024), (16384, 1024)])
def test_every_scatter_instantiation_two_rounds(hip_lib, oracle_lib, monkeypatch, T, NT):
    """Every instantiation ar_tiles_call can launch, forced: 6,000 groups x 3 = 18,000 votes are at least one whole tile
    (the 16-byte loads) and a partly filled one, whatever the shape.  Two rounds back to back: a load that went to the
    wrong place at the end of a tile or of the batch is a wrong vote in the round that follows."""
    monkeypatch.setenv("GPX_TILE_T", str(T))
    monkeypatch.setenv("GPX_TILE_NT", str(NT))
    G = 6000
    assert 3 * G > T and (3 * G) % T
    eh, eo = _pair(hip_lib, oracle_lib, G)
    g = np.arange(G, dtype=np.int32)
    for r in range(2):
        _propose_both(eh, eo, g)
        cols = _votes(G, r)
        eh.profile(2)
        dh, do = eh.accept_reply(*cols), eo.accept_reply(*cols)
        assert "k_scatter_tiles" in eh.profile_read()
        eh.profile(0)
        _same(dh, do, f"round {r}")
        assert dh.gidx.shape[0] == G
    assert eh.snapshot(g)[0].tobytes() == eo.snapshot(g)[0].tobytes()
    assert eh.counters() == eo.counters()
    eh.close(), eo.close()


def test_staging_is_read_back_after_an_in_place_call(hip_lib, oracle_lib):
    """In place, then a call that has to compact (one acceptor's votes withheld: every bucket decides another count than
    predicted, so k_emit_dec16 reads the staging the per-bucket kernel has just written beside its in-place stores),
    then in place again with the ratio learnt."""
    G = 6000
    eh, eo = _pair(hip_lib, oracle_lib, G)
    g = np.arange(G, dtype=np.int32)
    placed = 0
    for r, (what, want_placed) in enumerate([("all", True), ("lost", False), ("lost", True)]):
        _propose_both(eh, eo, g)
        cols = _votes(G, r)
        if what == "lost":
            keep = cols[4] != MEMBERS[-1]
            cols = [np.ascontiguousarray(c[keep]) for c in cols]
        _same(eh.accept_reply(*cols), eo.accept_reply(*cols), f"round {r} ({what})")
        p, c = eh.path_counters()
        assert p + c == r + 1
        assert (p == placed + 1) == want_placed, f"round {r} ({what}): in place {p}, compacted {c}"
        placed = p
    assert eh.snapshot(g)[0].tobytes() == eo.snapshot(g)[0].tobytes()
    assert eh.counters() == eo.counters()
    eh.close(), eo.close()


@pytest.mark.parametrize("kernel", ["k_propose_one", "k_propose_pers"])
def test_ordered_proposals_with_refusals_and_a_broken_promise(hip_lib, oracle_lib, monkeypatch, kernel):
    """Ordered proposal batches of 6,000 groups through the one-launch kernel and, with its bound forced to zero, through
    k_one_check + k_propose_one: accepted records, records refused because the window of 4 is full, and a batch whose
    promise breaks in the middle (everything from the descent on: GPX_S_UNORDERED and zero outputs) - all five output
    columns of every form against the oracle."""
    if kernel == "k_propose_one":
        monkeypatch.setenv("GPX_PERS_CHUNKS", "0,0,0")
    G = 6000
    eh, eo = _pair(hip_lib, oracle_lib, G, window=4)
    for e in (eh, eo):
        e.set_ordered_batches(ORDERED_PROPOSE)
    g = np.arange(G, dtype=np.int32)
    broken = g.copy()
    broken[G // 2] = broken[G // 2 - 1] - 5
    eh.profile(2)
    _propose_both(eh, eo, g, "first batch")
    st = _propose_both(eh, eo, broken, "broken promise")[4]
    assert (st[G // 2:] == S_UNORDERED).all() and not (st[:G // 2] == S_UNORDERED).any()
    for i in range(3):
        st = _propose_both(eh, eo, g, f"batch {i + 2}")[4]
    # (the first half has had one proposal more than the second: its fifth meets the full window)
    assert (st[:G // 2] == S_WINDOW).all() and (st[G // 2:] == S_OK).all()
    ran = eh.profile_read()
    assert kernel in ran and ("k_propose_pers" in ran) == (kernel == "k_propose_pers"), sorted(ran)
    assert eh.snapshot(g)[0].tobytes() == eo.snapshot(g)[0].tobytes()
    assert eh.counters() == eo.counters()
    eh.close(), eo.close()
