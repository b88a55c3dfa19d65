"""CPU checks of the test infrastructure behind test_geometry_gpu.py and test_backends_gpu.py: the geometry
restatement at the sizes the issue of those files names, the hot-set builder's placements, the fuzz driver's stream
with its default arguments (unchanged by the group map and minimum batch options), and the window legs of the fuzz
cells, run oracle against oracle."""
import numpy as np
import pytest

from gigapaxos_amd import S_WINDOW
from tests.fuzz_record import RecordingEngine
from tests.geometry_common import CELLS, RANGE, ar_route, geometry, hot_set, run_cell, tile_shape
from tests.parity_common import create_mixed_groups, fuzz, make_pair

NODES = [100, 101, 102, 103, 104, 105, 106, 107]


@pytest.mark.parametrize("G,shift,nbk,ac16,passes", [
    (130_560, 8, 510, True, 1), (130_561, 9, 256, True, 1), (1 << 21, 9, 4096, True, 1), ((1 << 21) + 1, 10, 2049, True, 1),
    (1 << 22, 10, 4096, True, 1), ((1 << 22) + 1, 11, 2049, False, 2), ((1 << 23) + 1, 12, 2049, False, 3),
    (10_000_000, 12, 2442, False, 3)])
def test_geometry_restatement(G, shift, nbk, ac16, passes):
    geo = geometry(G, 3)
    assert (geo["shift"], geo["nbk"], geo["ac16"], geo["ar_passes"]) == (shift, nbk, ac16, passes)
    assert geo["bucket_threads"] == min(1024, 1 << shift)
    assert geo["nbk16"] == (nbk if shift <= 10 else 4096)


def test_tile_shapes_at_4096_buckets():
    """4,096 buckets need nbk + 1 = 4,097 counters: a 512-thread scatter workgroup holds 4,096, so the 4,096-vote tile
    runs on 1,024 threads there; 1,954 buckets keep 512."""
    assert tile_shape(4096, 500_000) == (4096, 1024)
    assert tile_shape(4096, 3_100_000) == (12288, 1024)
    assert tile_shape(1954, 500_000) == (4096, 512)
    assert tile_shape(586, 600_000, 12288, 512) is None and tile_shape(586, 600_000, 16384, 512) is None
    assert tile_shape(4096, 600_000, 16384, 1024) is None  # the LDS of 16,384 votes and 8,192 counters
    assert ar_route(geometry(1 << 21, 3), 500_000)[0] == "tiles"
    assert ar_route(geometry((1 << 22) + 1, 3), 3_100_000) == ("partition", 2)
    assert ar_route(geometry(1 << 21, 3), 1024) == ("tiny",)


@pytest.mark.parametrize("G", [130_561, 1 << 21, (1 << 21) + 1, (1 << 22) + 1, (1 << 23) + 1, 3000, 9000])
def test_hot_set_covers_every_placement(G):
    shift = {3000: 11, 9000: 12}.get(G)
    geo = geometry(G, 3, shift)
    hot, place = hot_set(G, geo, np.random.default_rng(G))
    gb, nbk = geo["gb"], geo["nbk"]
    hs = set(hot.tolist())
    assert all(set(v.tolist()) <= hs for v in place.values())
    assert 0 in hs and G - 1 in hs and (nbk - 1) * gb in hs                         # first and last (partial) bucket
    cross = [b for b in range(1, nbk) if b * gb - 1 in hs and b * gb in hs]
    assert len(cross) >= min(nbk - 1, 8) and nbk - 1 in cross                       # both sides of bucket boundaries
    if G > RANGE:
        assert RANGE - 1 in hs and RANGE in hs                                      # ... and of the 2^22 range boundary
    if gb > 1024:
        b = (nbk - 1) // 2
        for l in (0, 1, 511, 1023):                                                 # one thread's lanes l, l + 1024, ...
            assert all(b * gb + l + j * 1024 in hs for j in range(gb // 1024))
    assert min(2000, G // 5) <= hot.shape[0] <= 6000


def _stream_hash(oracle_lib, kmax, G, seed, steps, ordered):
    rng = np.random.default_rng(seed)
    ea, eb = make_pair(oracle_lib, oracle_lib, 100, G, kmax, 64)
    ra = RecordingEngine(ea)
    create_mixed_groups(ra, eb, G, kmax, NODES, rng)
    fuzz(ra, eb, G, NODES, rng, steps=steps, batch=300, ordered=ordered)
    ea.close(), eb.close()
    return ra.hexdigest()


@pytest.mark.parametrize("kmax,G,seed,steps,ordered,digest", [
    (3, 64, 1, 250, False, "0d5e175d81b0536556b15201e92e382ec619eb0ff304c74419a8dccf396391b9"),
    (5, 64, 2, 250, False, "5169eb93a6b97f68c4f28fa37a64252260e3b24cb2a724f3e2bd6f9f963017f6"),
    (3, 48, 21, 160, True, "00725e47289b4e3cb18ffe2dbe04d77a87dc24ea21417a744e15de0f6853d4cc")])
def test_fuzz_default_stream_unchanged(oracle_lib, kmax, G, seed, steps, ordered, digest):
    """The streams of test_parity_gpu.py's seeds (mixed ops; grouped by group), hashed as the driver sent them before it
    took a group map and a minimum batch size."""
    assert _stream_hash(oracle_lib, kmax, G, seed, steps, ordered) == digest


def test_group_map_keeps_the_stream(oracle_lib):
    """The same seed through a group map: the same random draws, every record moved to its mapped row."""
    G, kmax = 64, 3
    gmap = np.sort(np.random.default_rng(5).choice(50_000, G, replace=False)).astype(np.int32)
    out = []
    for gm, Gt in ((None, G), (gmap, 50_000)):
        rng = np.random.default_rng(1)
        ea, eb = make_pair(oracle_lib, oracle_lib, 100, Gt, kmax, 64)
        create_mixed_groups(ea, eb, G, kmax, NODES, rng, gmap=gm)
        out.append(fuzz(ea, eb, G, NODES, rng, steps=120, batch=300, gmap=gm))
        rows = ea.snapshot(np.arange(G) if gm is None else gm)[0]
        out.append(rows.tobytes())
        ea.close(), eb.close()
    assert out[0] == out[2] and out[1] == out[3]


def test_windows_spread_over_the_cells():
    ws = {c["window"] for c in CELLS.values()}
    assert {4, 8, 32} <= ws
    assert {c["window"] for c in CELLS.values() if "propose" in c["refused"]} >= {4, 8}


@pytest.mark.parametrize("name", sorted(CELLS))
def test_window_cells_refuse(oracle_lib, name):
    seen, _ = run_cell(oracle_lib, oracle_lib, CELLS[name])
    for op in CELLS[name]["refused"]:
        assert S_WINDOW in seen[op], (name, op, seen)


@pytest.mark.parametrize("G,shift,limits", [(3000, 11, False), (3000, 11, True), (9000, 12, True)])
def test_wire_geometry_setup_and_first_pass_on_the_oracle(oracle_lib, G, shift, limits):
    """test_wire_geometry_gpu.py's setup binds every hot-set name, and its restatement of the device form's one pass
    (first_pass) agrees with the oracle's packer: frames, bytes and unbatched exactly where no per-call limit is hit;
    where one is, the records it marks 2 are packed by the host form's later passes and the rest match."""
    from gigapaxos_amd import wire as W
    from gigapaxos_amd import S_OK, hri_create
    from tests.test_wire_geometry_gpu import MEMBERS, hot_name, first_pass, _accept_batch
    geo = geometry(G, 3, shift)
    rng = np.random.default_rng(G)
    hot, place = hot_set(G, geo, rng)
    names = [hot_name(int(x)) for x in hot]
    assert len(set(names)) == hot.shape[0] and {len(x) for x in names} <= set(range(1, 128))
    e, _ = make_pair(oracle_lib, oracle_lib, 100, G, 3, 8)
    assert (e.create_groups(np.arange(G), np.tile(np.array(MEMBERS, np.int32), (G, 1)), 3, hri_create(G, 3, 100)) == S_OK).all()
    we = W.WireEngine(e)
    named_rows = np.setdiff1d(hot, hot[5::17]).astype(np.int32)
    assert (we.bind([hot_name(int(x)) for x in named_rows], named_rows) == S_OK).all()
    named = np.zeros(G, bool)
    named[named_rows] = True
    name_len = np.zeros(G, np.int32)
    name_len[named_rows] = [len(hot_name(int(x))) for x in named_rows]
    g, bnum, bcoord, slot, median, sender, big = _accept_batch(hot, place, G, rng)
    if not limits:
        keep = g != big
        g, bnum, bcoord, slot, median, sender = (x[keep] for x in (g, bnum, bcoord, slot, median, sender))
        bnum, bcoord = bnum % 2, 100 + bcoord % 2
        sender = np.where(sender == 100, 100, bcoord).astype(np.int32)
    (rb, rc, rm, _, st), _ = e.accept(g, bnum, bcoord, slot, median)
    ub, nf, nb = first_pass(g, st, sender, rb, rc, slot, named, name_len)
    frames, _, _, ub_o, nb_o = we.pack_accept_replies(g, slot, rb, rc, rm, st, sender)
    assert (ub == 1).any() and (ub == 0).any()
    if not limits:
        assert not (ub == 2).any()
        assert ub.tolist() == ub_o.tolist() and nf == len(frames) and nb == nb_o
    else:
        assert (ub[g == big] == 2).any()
        assert (ub_o[ub == 2] == 0).all() and ub_o[ub != 2].tolist() == ub[ub != 2].tolist()
        assert nf < len(frames) and nb < nb_o
    e.close()
