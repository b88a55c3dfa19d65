"""The journal batches (include/gpx_journal.h) on the GPU, bit for bit against tests/journal_model.py.  Every buffer of a
_dev call sits inside 4 KiB guard bands (tests/journal_common.py): `out` and the rows carry a sentinel that is checked
unchanged from bytes_done / row n_done to the end of the band, the frame block lies between bands of live, plausible
bytes, and refused frames show in n_bad and in the bytes - never as a fault.  Sizes are the smallest at which each
mechanism of the kernels can break."""
import numpy as np
import pytest

from gigapaxos_amd import Engine, hri_create, S_OK, wire as W
from tests import journal_common as JC
from tests import journal_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(hip_lib):
    e = Engine(hip_lib, 101, 64, kmax=3, window=8, max_batch=1 << 14)
    yield e
    e.close()


@pytest.mark.gpu_fast
@pytest.mark.parametrize("padded", [False, True])
def test_every_phase_of_a_boundary(eng, padded):
    """entry starts at every offset modulo 16, prefixes straddling a chunk in each way, source frames at every start
    offset modulo 16 (the block itself is moved through all sixteen), both frame forms"""
    lens = JC.phase_lengths()
    block, off, ln = JC.frames_of_lengths(lens, seed=21, padded=padded)
    cols = JC.all_logged_columns(len(lens))
    for mis in range(16):
        p = JC.pack_dev(eng, block, off, cols, frame_len=ln, misalign=mis, base_offset=(1 << 40) + mis, what="block at +%d" % mis)
        assert p.counts["n_done"] == 2000
        if mis >= 2 and not padded:
            break        # the contiguous form already has every source phase; two placements show the block may move


@pytest.mark.parametrize("k", [1, 2, 3])
def test_tile_edges(eng, k):
    """totals of 16384 k - 5 .. 16384 k + 5 whose last entry is a bare prefix: it ends at the tile boundary, is cut by
    it at each of its bytes, or starts at it"""
    rng = np.random.default_rng(k)
    for d in range(-5, 6):
        total, lens, t = 16384 * k + d, [], 0
        while total - t - 4 > 400:
            lens.append(97 + int(rng.integers(0, 50)))
            t += 4 + lens[-1]
        rest = total - t - 4
        lens += [rest // 2 - 4, rest - rest // 2 - 4, 0]
        assert sum(4 + x for x in lens) == total
        block, off, ln = JC.frames_of_lengths(lens, seed=100 * k + d + 5)
        p = JC.pack_dev(eng, block, off, JC.all_logged_columns(len(lens)), base_offset=77, what="total %d" % total)
        assert p.counts["bytes_done"] == total


def test_many_entries_per_tile_and_one_entry_over_many_tiles(eng):
    rng = np.random.default_rng(9)
    lens = rng.integers(0, 2, 10000).tolist()            # more than 4,096 descriptors in one 16 KB tile
    block, off, ln = JC.frames_of_lengths(lens, seed=31)
    JC.pack_dev(eng, block, off, JC.all_logged_columns(10000), what="10,000 entries of 0 and 1 bytes")
    block, off, ln = JC.frames_of_lengths([0] * 5000, seed=32, padded=True)
    JC.pack_dev(eng, block, off, JC.all_logged_columns(5000), frame_len=ln, what="5,000 empty frames")
    lens = [(1 << 20) + 13 if i == 1000 else int(rng.integers(0, 60)) for i in range(2001)]
    block, off, ln = JC.frames_of_lengths(lens, seed=33)
    p = JC.pack_dev(eng, block, off, JC.all_logged_columns(2001), base_offset=5, what="one entry of 1 MiB + 13 among 2,000")
    assert p.counts["n_done"] == 2001


def test_more_tiles_than_one_round_and_than_the_copy_grid(hip_lib):
    """70,000 records are 274 tiles of records, more than the 256 that one round of k_jr_offsets takes, and a cut by
    cap_entries falls into a tile of the second round; with frames of 720 bytes and more the journal has more than the
    2,048 output tiles the copy is launched with, so its workgroups come round a second time"""
    e = Engine(hip_lib, 101, 64, kmax=3, window=8, max_batch=70_000)
    n = 70_000
    lens = (720 + np.arange(n) % 21).tolist()
    block, off, _ = JC.frames_of_lengths(lens, seed=77)
    cols = JC.all_logged_columns(n)
    cols["r_flags"][::3] = M.R_STORED
    p = JC.pack_dev(e, block, off, cols, base_offset=1 << 35, what="70,000 records")
    assert p.counts["n_done"] == n - (n + 2) // 3 and p.counts["bytes_done"] > 2048 * 16384
    p = JC.pack_dev(e, block, off, cols, cap_entries=45_000, what="70,000 records, cut in tile 263")
    assert p.counts["n_done"] == 45_000
    e.close()


def test_selection_by_status_flag_and_frame_validity(eng):
    block, off, ln, rec_frame, cols = JC.selection_case()
    p = JC.pack_dev(eng, block, off, cols, frame_len=ln, rec_frame=rec_frame, base_offset=1000, what="selection")
    # logged: status OK with TOLOG (two flag values); usable frames 3, 7, 3 of the nine per combination
    assert (p.counts["n_entries"], p.counts["n_bad"]) == (2 * 3, 2 * 6)
    assert p.rows["rec"].tolist() == [i for i in range(len(rec_frame)) if cols["status"][i] == M.S_OK
                                      and cols["r_flags"][i] & M.R_TOLOG and rec_frame[i] in (3, 7)]
    # the decode form: an offset that runs backwards is a negative length
    block, off, _ = JC.frames_of_lengths([10 + i for i in range(40)], seed=5)
    off = off.copy()
    off[20] = off[21] + 5
    p = JC.pack_dev(eng, block, off, JC.all_logged_columns(40), what="offsets running backwards")
    assert p.counts["n_bad"] == 1 and p.counts["n_entries"] == 39


def test_caps_continuation_counts_only_and_empty_call(eng):
    rng = np.random.default_rng(12)
    lens = [21] + rng.integers(0, 90, 699).tolist()
    n = len(lens)
    block, off, _ = JC.frames_of_lengths(lens, seed=41)
    cols = JC.all_logged_columns(n)
    ends = np.cumsum([4 + x for x in lens]).tolist()
    whole = JC.pack_dev(eng, block, off, cols, base_offset=500, what="uncut")
    # cap_bytes: 0, one byte short of the first entry, exactly at an entry's end, one byte past it, inside a prefix
    for cb, k in ((0, 0), (24, 0), (25, 1), (ends[300], 301), (ends[300] + 1, 301), (ends[300] + 2, 301), (ends[300] + 3, 301),
                  (ends[255], 256), (ends[-1] - 1, n - 1)):
        p = JC.pack_dev(eng, block, off, cols, cap_bytes=cb, base_offset=9, what="cap_bytes %d" % cb)
        assert p.counts["n_done"] == k and p.counts["n_entries"] == n and p.counts["n_bytes"] == ends[-1]
    for ce in (0, 1, 256, n - 1):
        p = JC.pack_dev(eng, block, off, cols, cap_entries=ce, what="cap_entries %d" % ce)
        assert p.counts["n_done"] == ce and p.counts["bytes_done"] == (ends[ce - 1] if ce else 0)
    JC.pack_dev(eng, block, off, cols, cap_bytes=ends[400] + 2, cap_entries=300, null_rows=("rec", "gidx", "slot", "bnum", "bcoord"),
                what="both caps, the optional row columns NULL")
    # the cut call continued to the end: the concatenation is the uncut answer
    got, first, base = b"", 0, 500
    rec_frame = np.arange(n, dtype=np.int32)
    while first < n:
        part = {k: v[first:] for k, v in cols.items()}
        p = JC.pack_dev(eng, block, off, part, rec_frame=rec_frame[first:], cap_bytes=5000, cap_entries=64, base_offset=base,
                        what="continued from record %d" % first)
        assert p.counts["n_done"] > 0
        got += p.bytes
        base += p.counts["bytes_done"]
        first += int(p.rows["rec"][-1]) + 1
    assert got == whole.bytes and base == 500 + len(whole.bytes)
    p = JC.pack_dev(eng, block, off, cols, flags=M.COUNT_ONLY, what="counts only, NULL outputs")
    assert p.counts["n_done"] == 0 and p.counts["n_bytes"] == ends[-1]
    none = {k: v[:0] for k, v in cols.items()}
    for flags in (0, M.COUNT_ONLY):
        p = JC.pack_dev(eng, block, off, none, cap_bytes=64, cap_entries=4, flags=flags, what="n = 0")
        assert p.counts == dict(n_entries=0, n_done=0, n_bad=0, reserved=0, n_bytes=0, bytes_done=0)


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _journal_on_device(torch, e, n, d_frames, frames_bytes, n_frames, d_off, d_len, d_rec_frame, d_cols, d_rflags, d_status, base):
    """gpx_journal_pack_dev over columns that are already on the device -> (bytes, rows, counts)"""
    from gigapaxos_amd import journal as J
    cap = frames_bytes + 4 * n
    out = torch.full((cap + JC.GUARD,), JC.SENTINEL, dtype=torch.uint8, device="cuda")
    rows = {k: torch.full(((n + 8) * np.dtype(dt).itemsize,), JC.SENTINEL, dtype=torch.uint8, device="cuda") for k, dt in JC.ROW_DT.items()}
    cnt = torch.full((48,), JC.SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    J.journal_pack_dev(e, n, d_frames.data_ptr(), frames_bytes, n_frames, d_off.data_ptr(), d_len.data_ptr() if d_len is not None else 0,
                       d_rec_frame.data_ptr() if d_rec_frame is not None else 0, [c.data_ptr() for c in d_cols],
                       d_rflags.data_ptr(), d_status.data_ptr(), base, 0, out.data_ptr(), cap, n,
                       [rows[k].data_ptr() for k in JC.ROW_DT], cnt.data_ptr())
    e.sync()
    raw = cnt.cpu().numpy()
    assert (raw[32:] == JC.SENTINEL).all()
    counts = M.counts_of(J.JournalCounts.from_buffer_copy(raw[:32].tobytes()))
    o = out.cpu().numpy()
    assert (o[counts["bytes_done"]:] == JC.SENTINEL).all()
    r = {}
    for k, dt in JC.ROW_DT.items():
        a = rows[k].cpu().numpy()
        assert (a[counts["n_done"] * np.dtype(dt).itemsize:] == JC.SENTINEL).all(), k
        r[k] = a.view(dt)[:counts["n_done"]]
    return o[:counts["bytes_done"]].tobytes(), r, counts


def test_the_chain_decode_accept_journal_against_the_oracle(hip_lib, oracle_lib):
    """the five rounds of tests/test_journal_model.py through gpx_wire_decode_dev -> gpx_accept_batch_dev ->
    gpx_journal_pack_dev: nothing comes back to the host between the three; the oracle's r_flags / status decide the
    expected journal; the reader gets every logged frame back from the file the rounds build"""
    import torch
    eh, wh = JC.rounds_engine(hip_lib)
    eo, wo = JC.rounds_engine(oracle_lib)
    g, s = JC.round_records()
    n = g.size
    i32 = lambda k=n: torch.zeros(k, dtype=torch.int32, device="cuda")   # noqa: E731
    u8 = lambda k=n: torch.zeros(k, dtype=torch.uint8, device="cuda")    # noqa: E731
    P = lambda t: t.data_ptr()                                           # noqa: E731
    base, log, index = 0, b"", []
    for r, (bnum, bcoord) in enumerate(JC.ROUNDS):
        frames = JC.round_frames(g, s, bnum, bcoord)
        A, r_flags, status = JC.oracle_round(eo, wo, frames)
        buf, off = W.concat_frames(frames)
        d_buf, d_off = _dev(torch, buf), _dev(torch, off)
        acc = {k: i32() for k in ("gidx", "bnum", "bcoord", "slot", "median_cp", "sender", "frame")}
        acc["flags"], acc["req_id"] = u8(), torch.zeros(n, dtype=torch.int64, device="cuda")
        wc, fst, fg, ft = i32(8), u8(), i32(), i32()
        torch.cuda.synchronize()
        W.decode_dev(wh, n, P(d_buf), P(d_off), P(fst), P(fg), P(ft),
                     accepts=(n, [P(acc[k]) for k in ("gidx", "bnum", "bcoord", "slot", "median_cp", "flags", "sender", "req_id", "frame")]),
                     counts_ptr=P(wc))
        rb, rc, rm, rfl, st = i32(), i32(), i32(), u8(), u8()
        xg, xf, xc, nr = i32(), i32(), i32(), i32(1)
        eh.call_dev("accept_batch", n, P(acc["gidx"]), P(acc["bnum"]), P(acc["bcoord"]), P(acc["slot"]), P(acc["median_cp"]),
                    P(acc["flags"]), P(rb), P(rc), P(rm), P(rfl), P(st), P(xg), P(xf), P(xc), P(nr))
        got, rows, counts = _journal_on_device(torch, eh, n, d_buf, int(buf.shape[0]), n, d_off, None, acc["frame"],
                                               [acc[k] for k in ("gidx", "slot", "bnum", "bcoord")], rfl, st, base)
        assert int(wc[2]) == n and acc["frame"].cpu().numpy().tolist() == A["frame"].tolist()
        assert rfl.cpu().numpy().tolist() == r_flags.tolist() and st.cpu().numpy().tolist() == status.tolist()
        want = M.pack(buf, off, A["gidx"], A["slot"], A["bnum"], A["bcoord"], r_flags, status, rec_frame=A["frame"], base_offset=base)
        assert counts == want.counts and counts["n_done"] == JC.ROUND_LOGGED[r] and got == want.bytes, r
        for k in JC.ROW_DT:
            assert rows[k].tolist() == want.rows[k].tolist(), (r, k)
        log += got
        index += [(int(o), int(ln), frames[int(i)]) for o, ln, i in zip(rows["off"], rows["len"], rows["rec"])]
        base += counts["bytes_done"]
    assert len(index) == 4800 and base == len(log)
    for o, ln, frame in index:                          # the file of all five rounds, read as recovery reads it
        assert M.read_entry(log, o, ln) == frame
    assert M.walk(log)[2] == len(log)
    eh.close(), eo.close()


def test_the_coordinator_journals_its_own_accepts(hip_lib, oracle_lib):
    """the frame_len form: what gpx_wire_pack_accepts_dev wrote (4-byte aligned starts, pad bytes between the frames)
    is accepted and journalled by the coordinator's own acceptor"""
    import torch
    from tests import wire_accepts_model as WA
    G = 200
    engines = []
    for lib in (hip_lib, oracle_lib):
        e = Engine(lib, 100, G, kmax=3, window=8, max_batch=1 << 12)
        mem = np.tile(np.array([100, 101, 102], np.int32), (G, 1))
        assert (e.create_groups(np.arange(G), mem, 3, hri_create(G, 3, 100)) == S_OK).all()
        engines.append(e)
    eh, eo = engines
    wh = W.WireEngine(eh)
    names = [b"grp-%d" % q for q in range(G)]
    assert (wh.bind(names, np.arange(G)) == S_OK).all()
    rng = np.random.default_rng(17)
    reqs = [WA.random_request(rng, names[i % G], 0, 5000 + i, max_value=300) for i in range(2 * G)]
    r = WA.Chain(wh).run(reqs, batch=False)
    nF = r["n_frames"]
    # (a request with the stop flag ends its group: the proposals behind it get no frame)
    assert G < nF <= 2 * G and (r["frame_off"] % 4 == 0).all() and (r["frame_len"] % 4 != 0).any()
    b = r["f_batch"]
    cols = [r["f_gidx"], r["bnum"][b], r["bcoord"][b], r["slot"][b], r["median"][b]]
    (_, _, _, r_flags, status), _ = eo.accept(*cols)
    assert int(JC.logged(r_flags, status).sum()) >= nF // 2
    d = [_dev(torch, c.astype(np.int32)) for c in cols]
    i32 = lambda k=nF: torch.zeros(k, dtype=torch.int32, device="cuda")  # noqa: E731
    rfl, st = torch.zeros(nF, dtype=torch.uint8, device="cuda"), torch.zeros(nF, dtype=torch.uint8, device="cuda")
    outs = [i32(), i32(), i32(), rfl, st, i32(), i32(), i32(), i32(1)]
    flags = torch.zeros(nF, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eh.call_dev("accept_batch", nF, *[t.data_ptr() for t in d], flags.data_ptr(), *[t.data_ptr() for t in outs])
    block = r["out"][:r["n_bytes"]]
    got, rows, counts = _journal_on_device(torch, eh, nF, _dev(torch, block), int(block.shape[0]), nF, _dev(torch, r["frame_off"]),
                                           _dev(torch, r["frame_len"]), None, [d[0], d[3], d[1], d[2]], rfl, st, 4096)
    assert rfl.cpu().numpy().tolist() == r_flags.tolist() and st.cpu().numpy().tolist() == status.tolist()
    want = M.pack(block, r["frame_off"], cols[0], cols[3], cols[1], cols[2], r_flags, status, frame_len=r["frame_len"], base_offset=4096)
    assert counts == want.counts and got == want.bytes and counts["n_done"] == int(JC.logged(r_flags, status).sum())
    for k in JC.ROW_DT:
        assert rows[k].tolist() == want.rows[k].tolist(), k
    for e in range(counts["n_done"]):
        assert M.read_entry(got, int(rows["off"][e]), int(rows["len"][e]), 4096) == want.frames[e]
    eh.close(), eo.close()


def _host(e, block, off, cols, **kw):
    from gigapaxos_amd import journal as J
    out, rows, counts = J.journal_pack(e, block, off, cols["gidx"], cols["slot"], cols["bnum"], cols["bcoord"], cols["r_flags"],
                                       cols["status"], **kw)
    return (None if out is None else out.tobytes()), rows, M.counts_of(counts)


def _same_as_model(got, want):
    out, rows, counts = got
    assert counts == want.counts and out == want.bytes
    for k, a in zip(M.ROW_COLS, rows):
        assert a.tolist() == want.rows[k].tolist(), k


def test_host_twin_equals_the_device_form(eng):
    lens = JC.phase_lengths()
    for padded in (False, True):
        block, off, ln = JC.frames_of_lengths(lens, seed=21, padded=padded)
        cols = JC.all_logged_columns(len(lens))
        want = JC.pack_dev(eng, block, off, cols, frame_len=ln, base_offset=1 << 40)
        _same_as_model(_host(eng, block, off, cols, frame_len=ln, base_offset=1 << 40), want)
    block, off, ln, rec_frame, cols = JC.selection_case()
    want = JC.pack_dev(eng, block, off, cols, frame_len=ln, rec_frame=rec_frame, base_offset=1000)
    _same_as_model(_host(eng, block, off, cols, frame_len=ln, rec_frame=rec_frame, base_offset=1000), want)
    cut = JC.pack_dev(eng, block, off, cols, frame_len=ln, rec_frame=rec_frame, cap_entries=4, cap_bytes=200)
    _same_as_model(_host(eng, block, off, cols, frame_len=ln, rec_frame=rec_frame, cap_entries=4, cap_bytes=200), cut)
    out, rows, counts = _host(eng, block, off, cols, frame_len=ln, rec_frame=rec_frame, flags=M.COUNT_ONLY)
    assert out is None and counts == dict(want.counts, n_done=0, bytes_done=0)


def test_host_twin_in_chunks(hip_lib, monkeypatch):
    """a frame block forced through several chunks (a window of 64 KB instead of 64 MiB): the same bytes and rows,
    positions, record numbers and caps carried from chunk to chunk"""
    monkeypatch.setenv("GPX_TEST_JOURNAL_STAGE", "65536")
    e = Engine(hip_lib, 101, 64, kmax=3, window=8, max_batch=1 << 14)
    lens = JC.phase_lengths()                            # 253 KB of frames: four chunks
    block, off, ln = JC.frames_of_lengths(lens, seed=21, padded=True)
    cols = JC.all_logged_columns(len(lens))
    cols["r_flags"][::7] = M.R_STORED                    # some records are not logged
    rec_frame = np.arange(len(lens), dtype=np.int32)
    rec_frame[[5, 700, 1999]] = [-1, 2000, 3]            # two refused, one frame used twice
    mk = lambda **kw: M.pack(block, off, cols["gidx"], cols["slot"], cols["bnum"], cols["bcoord"], cols["r_flags"],   # noqa: E731
                             cols["status"], ln, rec_frame, **kw)
    assert block.shape[0] > 3 * 65536
    _same_as_model(_host(e, block, off, cols, frame_len=ln, rec_frame=rec_frame, base_offset=12345), mk(base_offset=12345))
    ends = (mk().rows["off"] + 4 + mk().rows["len"]).tolist()
    for cb, ce in ((ends[900] + 1, 5000), (1 << 30, 1200), (ends[3], 5000)):
        _same_as_model(_host(e, block, off, cols, frame_len=ln, rec_frame=rec_frame, cap_bytes=cb, cap_entries=ce),
                       mk(cap_bytes=cb, cap_entries=ce))
    e.close()


def test_the_profile_names_the_four_kernels(hip_lib):
    e = Engine(hip_lib, 101, 64, kmax=3, window=8, max_batch=1 << 12)
    block, off, _ = JC.frames_of_lengths([50] * 300, seed=2)
    cols = JC.all_logged_columns(300)
    e.profile(2)
    JC.pack_dev(e, block, off, cols, flags=M.COUNT_ONLY)
    prof0 = {k: v[0] for k, v in e.profile_read().items()}
    JC.pack_dev(e, block, off, cols)
    prof = {k: v[0] for k, v in e.profile_read().items()}
    e.profile(0)
    assert prof0 == {"k_jr_tile": 1, "k_jr_offsets": 1}, prof0
    assert prof == {"k_jr_tile": 2, "k_jr_offsets": 2, "k_jr_rows": 1, "k_jr_copy": 1}, prof
    e.close()
