"""Packed 8-byte vote records (include/gpx_packed.h), the part that needs no GPU: the header, the exported symbols and
the binding, and the host helpers gpx_votes_pack / gpx_votes_unpack against the numpy restatement of
tests/packed_model.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from gigapaxos_amd import streams
from tests import packed_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE_CALLS = ("gpx_votes_unpack_dev", "gpx_accept_reply_packed_dev", "gpx_accept_reply_packed_async")
HELPERS = ("gpx_votes_pack", "gpx_votes_unpack")
MEMBERS = [100, 101, 102]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from gigapaxos_amd import load_hip

    return load_hip()


def _pack(lib, cols, **kw):
    from gigapaxos_amd.packed import pack_votes

    return pack_votes(cols, lib=lib, **kw)


def _unpack(lib, p):
    from gigapaxos_amd.packed import unpack_votes

    return unpack_votes(p, lib=lib)


def _hdr(p):
    return dict(n=p.n, n_exc=p.n_exc, bnum=p.bnum, bcoord=p.bcoord, base_slot=p.base_slot, base_cp=p.base_cp,
                base_acceptor=p.base_acceptor)


def _same_cols(a, b, what):
    assert len(a) == len(b) == 6
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == np.int32 and x.shape == y.shape and (x == y).all(), f"{what}: column {k}"


def _batches():
    rng = np.random.default_rng(20250)
    out = {
        "vote_round": streams.vote_round(3000, MEMBERS, 2, 100),
        "vote_round mix": streams.vote_round(3000, MEMBERS, 3, 100, mix=True),
        "straddles MAX_VALUE": M.wrap_batch(5000, rng, 2**31 - 1),
        "straddles MIN_VALUE": M.wrap_batch(5000, rng, -2**31),
        "nodes 2^20 apart": M.far_nodes_batch(4000, rng),
        "odd first vote": M.odd_first_batch(2000),
        "own slots": M.own_slot_batch(3000),
    }
    for n in (0, 1, 3, 4, 5):
        out[f"n={n}"] = tuple(c[:n].copy() for c in streams.vote_round(2, MEMBERS, 0, 100, mix=True))
        assert out[f"n={n}"][0].shape[0] == n
    return out


BATCHES = _batches()


def test_header_library_and_binding_agree(lib):
    """The three engine calls and the two helpers are declared in include/gpx_packed.h (and nowhere in gpx.h /
    gpx_wire.h, whose names the oracle must mirror), exported by the built library and bound by _abi.py."""
    from gigapaxos_amd import _abi

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpx_packed.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gpx_[a-z_]+)\s*\(", src))
    assert declared == set(ENGINE_CALLS + HELPERS)
    for hdr in ("gpx.h", "gpx_wire.h"):
        other = open(os.path.join(ROOT, "include", hdr)).read()
        assert not any(name in other for name in declared), hdr
    raw = ctypes.CDLL(lib.path)
    for name in declared:
        assert hasattr(raw, name), name
        assert name[4:] in _abi.EXPORTED_SYMBOLS and name[4:] in lib.fn
    for name in ENGINE_CALLS:
        assert name[4:] in _abi._DEV_SIGS
    assert ctypes.sizeof(_abi.GpxPackedVotes) == 48
    for m in ("accept_reply_packed_async", "accept_reply_packed_dev", "votes_unpack_dev"):
        assert callable(getattr(_abi.Engine, m))


@pytest.mark.parametrize("name", list(BATCHES))
def test_unpack_of_pack_is_the_batch(lib, name):
    cols = BATCHES[name]
    n = cols[0].shape[0]
    p = _pack(lib, cols, exc_cap=n)
    assert p.needed == p.n_exc and p.n == n
    _same_cols(_unpack(lib, p), cols, name)
    # ... and through the model, both ways round
    _same_cols(M.unpack(_hdr(p), p.rec, p.exc), cols, name + " (model unpack of C pack)")
    hdr, rec, exc = M.pack(cols)
    _same_cols(M.unpack(hdr, rec, exc), cols, name + " (model)")


@pytest.mark.parametrize("name", list(BATCHES))
def test_c_packer_equals_model_byte_for_byte(lib, name):
    cols = BATCHES[name]
    assert cols[0].shape[0] <= 10_000
    p = _pack(lib, cols, exc_cap=cols[0].shape[0])
    hdr, rec, exc = M.pack(cols)
    assert _hdr(p) == hdr
    assert p.rec.tobytes() == rec.tobytes()
    assert p.exc.tobytes() == exc.tobytes()


def test_exception_counts_follow_from_the_stream(lib):
    """vote_round: one ballot, one slot, three node ids -> no exception; with mix exactly the votes whose ballot is not
    (0, coordinator) - the ns_ + nh stale and higher-ballot extras of streams.vote_round, under 1 % of the call."""
    for G, r in ((3000, 0), (40_000, 5)):
        cols = streams.vote_round(G, MEMBERS, r, 100)
        assert _pack(lib, cols).needed == 0
        cols = streams.vote_round(G, MEMBERS, r, 100, mix=True)
        n = G * 3
        ns_, nh = max(1, n // 200), max(1, n // 1000)
        p = _pack(lib, cols)
        assert p.needed == p.n_exc == int(((cols[1] != 0) | (cols[2] != 100)).sum()) == ns_ + nh
        assert p.n_exc * 100 < p.n and (p.bnum, p.bcoord) == (0, 100)
        assert p.nbytes == 8 * p.n + 32 * p.n_exc
    # a batch across the wrap: every delta stays within -128 .. +127 of the first vote in uint32 arithmetic
    for name in ("straddles MAX_VALUE", "straddles MIN_VALUE"):
        assert np.ptp(BATCHES[name][3].astype(np.int64)) > 2**31 and _pack(lib, BATCHES[name]).needed == 0
    # an odd first vote costs one row, not n - 1; every group at its own slot: all but those within a byte of the first
    assert _pack(lib, M.odd_first_batch(2000), exc_cap=2000).needed == 1
    p = _pack(lib, M.own_slot_batch(3000), exc_cap=3000)
    assert (p.base_slot, p.needed) == (-128, 3000 - 13)   # deltas 128 + 10 g <= 255: g = 0 .. 12


def test_capacity_too_small_writes_nothing_past_it(lib):
    cols = M.own_slot_batch(3000)
    full = _pack(lib, cols, exc_cap=3000)
    cap = 100
    exc = np.full(8 * (cap + 50), 0x5A5A5A5A, np.int32)
    rec = np.zeros(2 * 3000, np.uint32)
    p = _pack(lib, cols, exc_cap=cap, rec_out=rec, exc_out=exc[:8 * cap])
    assert p.needed == full.needed > cap and p.n_exc == cap
    assert (exc[8 * cap:] == 0x5A5A5A5A).all()
    assert exc[:8 * cap].tobytes() == full.exc[:cap].tobytes()
    assert p.rec.tobytes() == full.rec.tobytes()
    # the votes whose rows did not fit read as malformed; the others are intact
    got = _unpack(lib, p)
    lost = ((p.rec[:, 1] & M.EXC_BIT) != 0) & ((p.rec[:, 1] & ~M.EXC_BIT) >= cap)
    assert int(lost.sum()) == full.needed - cap and (got[0][lost] == -1).all()
    _same_cols([c[~lost] for c in got], [c[~lost] for c in cols], "rows that fit")
    # no capacity at all, no buffer
    assert _pack(lib, cols, exc_cap=0).needed == full.needed


def test_pack_and_unpack_reject_bad_arguments(lib):
    from gigapaxos_amd._abi import GpxPackedVotes

    pv = GpxPackedVotes()
    arrays = streams.vote_round(4, MEMBERS, 0, 100)
    rec_a = np.zeros(24, np.uint32)
    cols = [c.ctypes.data_as(ctypes.c_void_p) for c in arrays]
    rec = rec_a.ctypes.data_as(ctypes.c_void_p)
    assert lib.fn["votes_pack"](-1, *cols, rec, None, 0, ctypes.byref(pv)) == -1
    assert lib.fn["votes_pack"](12, *cols, None, None, 0, ctypes.byref(pv)) == -1
    assert lib.fn["votes_pack"](12, *cols, rec, None, 4, ctypes.byref(pv)) == -1
    assert lib.fn["votes_pack"](12, *cols, rec, None, 0, None) == -1
    assert lib.fn["votes_pack"](12, *cols, rec, None, 0, ctypes.byref(pv)) == 0
    assert lib.fn["votes_unpack"](None, *cols) == -1
    pv.n_exc = 1                                            # rows promised, none given
    assert lib.fn["votes_unpack"](ctypes.byref(pv), *cols) == -1


def test_malformed_records_unpack_to_no_group(lib):
    """Reserved bits set, or a row index >= n_exc: gidx = -1 for that record, every other record as before."""
    rng = np.random.default_rng(7)
    cols = streams.vote_round(2000, MEMBERS, 4, 100, mix=True)
    p = _pack(lib, cols)
    assert p.n_exc > 0
    rec, idx = M.malformed(p.rec, p.n_exc, rng, 40)
    from gigapaxos_amd.packed import PackedVotes

    q = PackedVotes(p.n, p.n_exc, p.bnum, p.bcoord, p.base_slot, p.base_cp, p.base_acceptor, rec, p.exc)
    got = _unpack(lib, q)
    _same_cols(got, M.unpack(_hdr(q), rec, p.exc), "malformed: C against model")
    bad = np.zeros(p.n, bool)
    bad[idx] = True
    assert (got[0][bad] == -1).all() and all((c[bad] == 0).all() for c in got[1:])
    _same_cols([c[~bad] for c in got], [c[~bad] for c in cols], "neighbours of malformed records")
    # an exception row named twice is fine: both records read it
    rec2 = p.rec.copy()
    e = np.nonzero(rec2[:, 1] & M.EXC_BIT)[0]
    rec2[e[1], 1] = rec2[e[0], 1]
    q2 = PackedVotes(p.n, p.n_exc, p.bnum, p.bcoord, p.base_slot, p.base_cp, p.base_acceptor, rec2, p.exc)
    got2 = _unpack(lib, q2)
    assert [int(c[e[1]]) for c in got2[1:]] == [int(c[e[0]]) for c in cols[1:]] and got2[0][e[1]] == cols[0][e[1]]
