"""The journal batches (include/gpx_journal.h) without a GPU: the model of tests/journal_model.py read back by the
reader written from getJournaledMessage; gpx_journal_walk against that reader on whole and torn buffers; and the five
ACCEPT rounds on the CPU oracle, whose log flags decide what the GPU leg (tests/test_journal_gpu.py) must journal - so
that leg cannot pass on an empty journal."""
import numpy as np
import pytest

from tests import journal_common as JC
from tests import journal_model as M


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from gigapaxos_amd import load_hip

    return load_hip()


@pytest.mark.parametrize("padded", [False, True])
def test_the_reader_gets_the_selected_frames_back_row_by_row(padded):
    lens = JC.phase_lengths()[:600]
    block, off, ln = JC.frames_of_lengths(lens, seed=11, padded=padded)
    n = len(lens)
    rng = np.random.default_rng(5)
    cols = JC.all_logged_columns(n)
    cols["status"] = rng.choice(np.array([M.S_OK, M.S_OK, M.S_WINDOW, M.S_NOGROUP], np.uint8), n)
    cols["r_flags"] = rng.integers(0, 4, n).astype(np.uint8)
    rec_frame = rng.permutation(n).astype(np.int32)
    rec_frame[::50] = -1                                 # refused: counted, no entry
    base = 123456789012
    p = M.pack(block, off, cols["gidx"], cols["slot"], cols["bnum"], cols["bcoord"], cols["r_flags"], cols["status"], ln,
               rec_frame, base_offset=base)
    sel = [i for i in range(n) if cols["status"][i] == M.S_OK and cols["r_flags"][i] & M.R_TOLOG]
    good = [i for i in sel if rec_frame[i] >= 0]
    assert len(good) > 100 and p.counts["n_bad"] == len(sel) - len(good) > 0
    assert p.counts["n_entries"] == p.counts["n_done"] == len(good) and p.rows["rec"].tolist() == good
    blob = block.tobytes()
    for e, i in enumerate(good):
        f = int(rec_frame[i])
        frame = blob[int(off[f]):int(off[f]) + lens[f]]
        assert M.read_entry(p.bytes, int(p.rows["off"][e]), int(p.rows["len"][e]), base) == frame
        assert (p.rows["gidx"][e], p.rows["slot"][e], p.rows["bnum"][e], p.rows["bcoord"][e]) == \
            (cols["gidx"][i], cols["slot"][i], cols["bnum"][i], cols["bcoord"][i])
    assert p.bytes == M.logbatch(p.frames)                               # FileLogger::logBatch's loop; no pad byte
    # the caps: a prefix, cut where the first entry does not fit
    ends = (p.rows["off"] - base + 4 + p.rows["len"]).tolist()
    for cb, ce in ((0, n), (ends[0] - 1, n), (ends[0], n), (ends[40] + 2, n), (ends[-1], 17), (ends[-1], 0)):
        q = M.pack(block, off, cols["gidx"], cols["slot"], cols["bnum"], cols["bcoord"], cols["r_flags"], cols["status"], ln,
                   rec_frame, base_offset=base, cap_bytes=cb, cap_entries=ce)
        k = min(ce, sum(1 for x in ends if x <= cb))
        assert q.counts["n_done"] == k and q.bytes == p.bytes[:ends[k - 1] if k else 0]
        assert q.counts["n_entries"] == len(good) and q.counts["n_bytes"] == len(p.bytes)
    q = M.pack(block, off, cols["gidx"], cols["slot"], cols["bnum"], cols["bcoord"], cols["r_flags"], cols["status"], ln,
               rec_frame, flags=M.COUNT_ONLY)
    assert q.bytes == b"" and q.rows is None and q.counts["n_done"] == 0 and q.counts["n_bytes"] == len(p.bytes)


def test_walk_and_reader_agree_on_whole_and_torn_buffers(lib):
    from gigapaxos_amd import journal as J

    frames = [b"", b"a", b"abc", b"abcd", b"abcde", bytes(range(256)) * 3, b"", b"tail-entry"]
    whole = M.logbatch(frames)
    base = 1 << 33
    offs, lens, good = M.walk(whole, base)
    assert lens == [len(f) for f in frames] and good == len(whole)
    e_off, e_len, n, gb = J.journal_walk(whole, base, lib=lib)
    assert (e_off.tolist(), e_len.tolist(), n, gb) == (offs, lens, len(frames), len(whole))
    for o, ln, f in zip(offs, lens, frames):
        assert M.read_entry(whole, o, ln, base) == f
    # a torn tail, cut at every byte of the last entry: the walk stops in front of it
    last = len(whole) - 4 - len(frames[-1])
    for cut in range(last, len(whole)):
        e_off, e_len, n, gb = J.journal_walk(whole[:cut], base, lib=lib)
        assert (n, gb) == (len(frames) - 1, last) and e_off.tolist() == offs[:-1], cut
        assert M.walk(whole[:cut], base) == (offs[:-1], lens[:-1], last)
    # a negative length is a torn entry; rows for the first `cap` only, all whole entries counted; an empty buffer
    e_off, e_len, n, gb = J.journal_walk(whole[:offs[3] - base] + b"\xff\xff\xff\xfe" + b"x" * 20, base, lib=lib)
    assert (n, gb) == (3, offs[3] - base)
    e_off, e_len, n, gb = J.journal_walk(whole, base, cap=2, lib=lib)
    assert (e_off.tolist(), e_len.tolist(), n, gb) == (offs[:2], lens[:2], len(frames), len(whole))
    assert J.journal_walk(b"", 5, lib=lib)[2:] == (0, 0) and M.walk(b"", 5) == ([], [], 0)


def test_the_five_rounds_log_what_the_issue_says_on_the_oracle(oracle_lib):
    """ballot (0, 100): the window refuses a third, the rest is logged; the same again: answered, nothing logged; a
    higher ballot: logged again; the lower ballot again: every record answered (NACKs), nothing logged - the case that
    tells the flag from the status; the higher one again: nothing"""
    eo, wo = JC.rounds_engine(oracle_lib)
    g, s = JC.round_records()
    base = 0
    for r, (bnum, bcoord) in enumerate(JC.ROUNDS):
        frames = JC.round_frames(g, s, bnum, bcoord)
        A, r_flags, status = JC.oracle_round(eo, wo, frames)
        assert (A["gidx"] == g).all() and (A["slot"] == s).all() and (A["frame"] == np.arange(g.size)).all()
        sel = JC.logged(r_flags, status)
        assert int((status == M.S_OK).sum()) == JC.ROUND_OK[r] and int(sel.sum()) == JC.ROUND_LOGGED[r], r
        if r == 0:
            assert 2 * int(sel.sum()) >= g.size              # at least half of the records are logged
        block, off = np.frombuffer(b"".join(frames), np.uint8), np.cumsum([0] + [len(f) for f in frames])
        p = M.pack(block, off, A["gidx"], A["slot"], A["bnum"], A["bcoord"], r_flags, status, rec_frame=A["frame"],
                   base_offset=base)
        assert p.counts["n_done"] == JC.ROUND_LOGGED[r] and p.counts["n_bad"] == 0
        assert p.frames == [frames[i] for i in np.nonzero(sel)[0]]
        for e in range(p.counts["n_done"]):
            assert M.read_entry(p.bytes, int(p.rows["off"][e]), int(p.rows["len"][e]), base) == p.frames[e]
        base += p.counts["bytes_done"]
    assert base > 2 * 2400 * 100
    eo.close()
