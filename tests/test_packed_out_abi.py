"""Packed proposal and decision outputs (include/gpx_packed_out.h), the part that needs no GPU: the header, the exported
symbols and the binding; the host packers and unpackers against the numpy restatement of tests/packed_out_model.py,
byte for byte over the whole used size; and the proof, on the CPU oracle alone, that the inputs of the GPU tests bring
about the forms they are chosen for."""
import ctypes
import os
import re

import numpy as np
import pytest

from gigapaxos_amd import Engine, streams, S_OK
from tests import packed_out_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE_CALLS = ("gpx_decisions_pack_dev", "gpx_proposals_pack_dev", "gpx_propose_packed_out_async",
                "gpx_accept_reply_packed_io_async")
HELPERS = ("gpx_packed_out_size", "gpx_decisions_pack", "gpx_proposals_pack", "gpx_decisions_unpack",
           "gpx_proposals_unpack")
KINDS = {"decisions": M.DECISIONS, "proposals": M.PROPOSALS}
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from gigapaxos_amd import load_hip

    return load_hip()


def c_pack(lib, kind, cols, slack=64):
    """The C packer into a sentinel-filled buffer of GPX_PACKED_OUT_BYTES(n) + slack -> (PackedOut, whole array)"""
    from gigapaxos_amd.packed_out import pack_decisions, pack_proposals, packed_out_bytes

    n = len(cols[-1])
    assert packed_out_bytes(n) == M.out_bytes(n)
    buf = np.full(M.out_bytes(n) + slack, SENTINEL, np.uint8)
    p = (pack_decisions if kind == M.DECISIONS else pack_proposals)(cols, lib=lib, out=buf[:M.out_bytes(n)])
    return p, buf


def c_unpack(lib, kind, buf, nbytes=None):
    from gigapaxos_amd.packed_out import unpack_decisions, unpack_proposals

    return (unpack_decisions if kind == M.DECISIONS else unpack_proposals)(buf, lib=lib, nbytes=nbytes)


def same_cols(a, b, what):
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        x, y = np.asarray(x), np.asarray(y)
        assert x.dtype == y.dtype and x.shape == y.shape and (x == y).all(), f"{what}: column {k}"


def check_against_model(lib, kind, cols, what):
    """C pack == model pack over the whole used size, nothing written past it, unpack(pack(cols)) == cols both ways"""
    cols = [np.ascontiguousarray(c, np.uint8 if k == len(cols) - 1 else np.int32) for k, c in enumerate(cols)]
    p, buf = c_pack(lib, kind, cols)
    model, hdr, needed = M.pack(kind, cols)
    assert p.header() == hdr, what
    assert p.needed == needed == M.needed_rows(kind, cols), what
    assert p.nbytes == model.shape[0] == M.used_size(hdr), what
    assert buf[:p.nbytes].tobytes() == model.tobytes(), what
    assert (buf[p.nbytes:] == SENTINEL).all(), f"{what}: bytes written past gpx_packed_out_size"
    same_cols(c_unpack(lib, kind, buf[:p.nbytes]), cols, what + " (C unpack)")
    same_cols(M.unpack(kind, model), cols, what + " (model unpack)")
    return p


# ---- the oracle's own outputs -----------------------------------------------------------------------------------------
def oracle_rounds(G, k, rounds, case=None, mix_round=3):
    """[(proposal columns, decision columns, vote columns)] per round of the CPU oracle; `case` = A / B / C inputs"""
    from tests.oracle_binding import load_oracle

    members = list(range(100, 100 + k))
    eo = Engine(load_oracle(), 100, G, kmax=k, window=8, max_batch=G * k + G * k // 40 + 4096)
    mem = np.tile(np.array(members, np.int32), (G, 1))
    assert (eo.create_groups(np.arange(G), mem, k, M.ahead_rows(case, G, k, 100)) == S_OK).all()
    g = np.arange(G, dtype=np.int32)
    out = []
    for r in range(rounds):
        po = eo.propose(g)
        votes = M.ahead_votes(case, G, members, r, 100, mix=(r == mix_round))
        d = eo.accept_reply(*votes)
        out.append((list(po), [d.gidx, d.slot, d.bnum, d.bcoord, d.median_cp, d.kind], votes))
    eo.close()
    return out


@pytest.fixture(scope="module")
def plain_rounds():
    return {(G, k): oracle_rounds(G, k, 6) for G, k in ((3000, 3), (100_000, 5))}


@pytest.fixture(scope="module")
def case_rounds():
    return {case: oracle_rounds(3000, 3, 2, case=case, mix_round=-1) for case in "ABC"}


def test_header_library_and_binding_agree(lib):
    from gigapaxos_amd import _abi

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpx_packed_out.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gpx_[a-z_]+)\s*\(", src))
    assert declared == set(ENGINE_CALLS + HELPERS)
    for hdr in ("gpx.h", "gpx_wire.h", "gpx_packed.h"):
        other = open(os.path.join(ROOT, "include", hdr)).read()
        assert not any(name in other for name in declared), hdr
    raw = ctypes.CDLL(lib.path)
    for name in declared:
        assert hasattr(raw, name), name
        assert name[4:] in _abi.EXPORTED_SYMBOLS and name[4:] in lib.fn
    for name in ENGINE_CALLS:
        assert name[4:] in _abi._DEV_SIGS
    for name in HELPERS:
        assert name[4:] in _abi._HOST_SIGS
    assert ctypes.sizeof(_abi.GpxPackedOutHdr) == 32
    assert re.search(r"int32_t form;.*int32_t kind;.*int32_t n;.*int32_t n_exc;.*int32_t bnum, bcoord, base_slot, base_cp;",
                     src, flags=re.S)
    for m in ("propose_packed_out_async", "accept_reply_packed_io_async", "decisions_pack_dev", "proposals_pack_dev"):
        assert callable(getattr(_abi.Engine, m))
    for cap in (0, 1, 7, 8, 9, 3000, 1 << 20):
        assert M.out_bytes(cap) == 32 + 5 * M.R(4 * cap) + M.R(cap)


@pytest.mark.parametrize("kind", list(KINDS))
def test_packers_equal_the_model_on_synthetic_columns(lib, kind):
    K = KINDS[kind]
    forms = {}
    for name, cols in M.synthetic_cases(K).items():
        forms[name] = check_against_model(lib, K, cols, f"{kind}, {name}")
    assert forms["straddles MAX_VALUE"].needed == forms["straddles MIN_VALUE"].needed == 0
    assert forms["odd first entry"].needed == 1 and forms["odd first entry"].bcoord == 100   # one row, not n - 1
    assert forms["tie among the first 64 (first entry's ballot wins)"].bcoord == 101
    assert forms["tie among the first 64 (the other way round)"].bcoord == 100
    assert forms["entries of another ballot"].n_exc == 40 and forms["entries of another ballot"].form == M.RECORDS
    p = forms["n=0"]
    assert p.header() == dict(form=M.RECORDS, kind=K, n=0, n_exc=0, bnum=0, bcoord=0, base_slot=0, base_cp=0) and p.nbytes == 32
    for n in (4000, 4003):                                    # the form boundary
        a, b = forms[f"n={n}, n // 4 rows"], forms[f"n={n}, n // 4 + 1 rows"]
        assert (a.form, a.n_exc, a.needed) == (M.RECORDS, n // 4, n // 4)
        assert (b.form, b.n_exc, b.needed) == (M.COLUMNS, 0, n // 4 + 1)
        assert a.nbytes <= 16 * n + 64 and b.nbytes <= M.out_bytes(n)
    if K == M.PROPOSALS:
        st = c_unpack(lib, K, forms["every status value"].raw)[4]
        assert sorted(set(st.tolist())) == list(range(256))


@pytest.mark.parametrize("G,k", [(3000, 3), (100_000, 5)])
def test_packers_equal_the_model_on_the_oracles_rounds(lib, plain_rounds, G, k):
    """Every proposal and every decision of every round carries one ballot and lies within a byte of the reference: no
    row, 4 bytes per proposal and 8 per decision - round 3, the adversarial mix, included."""
    for r, (po, dec, _) in enumerate(plain_rounds[(G, k)]):
        p = check_against_model(lib, M.PROPOSALS, po, f"round {r} proposals")
        d = check_against_model(lib, M.DECISIONS, dec, f"round {r} decisions")
        assert (p.form, p.n_exc, p.n) == (M.RECORDS, 0, G) and p.nbytes == 32 + M.R(4 * G)
        assert (d.form, d.n_exc) == (M.RECORDS, 0) and d.nbytes == 32 + M.R(8 * d.n) and d.n >= G - G // 50


# what the GPU tests assert of the raw buffers, per case: (form, n_exc, needed) of proposals and of decisions, rows the votes need
EXPECTED = {"A": ((M.RECORDS, 300, 300), (M.RECORDS, 300, 300), 900),
            "B": ((M.COLUMNS, 0, 999), (M.COLUMNS, 0, 999), 0),
            "C": ((M.COLUMNS, 0, 1500), None, 4500)}


@pytest.mark.parametrize("case", list(EXPECTED))
def test_gpu_inputs_bring_about_the_forms_they_are_chosen_for(lib, case_rounds, case):
    from gigapaxos_amd.packed import pack_votes

    exp_p, exp_d, exp_votes = EXPECTED[case]
    for r, (po, dec, votes) in enumerate(case_rounds[case]):
        p = check_against_model(lib, M.PROPOSALS, po, f"case {case} round {r} proposals")
        assert (p.form, p.n_exc, p.needed) == exp_p and p.n == 3000
        pv = pack_votes(votes, lib=lib, exc_cap=9000)
        assert pv.needed == exp_votes and (pv.needed <= 9000 // 4) == (case != "C")
        assert (po[4] == S_OK).all()
        if exp_d is not None:
            d = check_against_model(lib, M.DECISIONS, dec, f"case {case} round {r} decisions")
            assert (d.form, d.n_exc, d.needed) == exp_d and d.n == 3000


def test_short_buffers_and_bad_arguments_are_refused(lib):
    cols = M.steady(M.DECISIONS, 100)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    buf = np.full(M.out_bytes(100), SENTINEL, np.uint8)
    args = [ptr(c) for c in cols]
    assert lib.fn["decisions_pack"](100, *args, ptr(buf), M.out_bytes(100) - 1) == -2
    assert lib.fn["proposals_pack"](100, *args[1:], ptr(buf), M.out_bytes(100) - 1) == -2
    assert (buf == SENTINEL).all()
    assert lib.fn["decisions_pack"](-1, *args, ptr(buf), buf.nbytes) == -1
    assert lib.fn["decisions_pack"](100, *args, None, buf.nbytes) == -1
    assert lib.fn["decisions_pack"](100, None, *args[1:], ptr(buf), buf.nbytes) == -1
    assert lib.fn["proposals_pack"](100, *args[1:5], None, ptr(buf), buf.nbytes) == -1
    bad_kind = [c.copy() for c in cols]
    bad_kind[5][3] = 4                                          # d_kind has two bits
    assert lib.fn["decisions_pack"](100, *[ptr(c) for c in bad_kind], ptr(buf), buf.nbytes) == -1
    assert lib.fn["decisions_pack"](100, *args, ptr(buf), buf.nbytes) == 0
    assert lib.fn["packed_out_size"](ptr(buf)) == 32 + M.R(800)
    assert lib.fn["packed_out_size"](None) == -1
    # the columns of the caller are too short for the buffer
    outs = [np.zeros(50, np.int32) for _ in range(5)] + [np.zeros(50, np.uint8)]
    n = ctypes.c_int32(-7)
    assert lib.fn["decisions_unpack"](ptr(buf), buf.nbytes, 50, *[ptr(c) for c in outs], ctypes.byref(n)) == -2
    assert n.value == -7 and all((c == 0).all() for c in outs)


@pytest.mark.parametrize("kind", list(KINDS))
def test_corrupted_buffers_are_refused_whole(lib, kind):
    """Bad form, bad kind, a reserved bit, a row index >= n_exc, a truncated length: GPX_EINVAL from the C unpacker (and
    a ValueError from the model), and not one entry written."""
    from gigapaxos_amd._abi import GpxError

    K = KINDS[kind]
    n = 1000
    good, _ = c_pack(lib, K, M.with_rows(K, n, [5, 17, 600]))[0], None
    raw = good.raw.copy()
    assert good.form == M.RECORDS and good.n_exc == 3
    wstride, woff = (8, 4) if K == M.DECISIONS else (4, 0)

    def word(buf, i):
        return buf[32 + wstride * i + woff:32 + wstride * i + woff + 4].view(np.uint32)

    broken = {}
    for name, form in (("form 0", 0), ("form 3", 3)):
        b = raw.copy()
        b[0:4].view(np.int32)[0] = form
        broken[name] = (b, None)
    b = raw.copy()
    b[4:8].view(np.int32)[0] = 3 - K
    broken["the other kind"] = (b, None)
    b = raw.copy()
    b[4:8].view(np.int32)[0] = 7
    broken["unknown kind"] = (b, None)
    b = raw.copy()
    word(b, 900)[0] |= np.uint32(1 << 30)
    broken["reserved bit 30"] = (b, None)
    b = raw.copy()
    word(b, 901)[0] |= np.uint32(1 << (18 if K == M.DECISIONS else 24))
    broken["lowest reserved bit"] = (b, None)
    b = raw.copy()
    word(b, 17)[0] = np.uint32(M.EXC_BIT | 3)
    broken["row index == n_exc"] = (b, None)
    broken["truncated by a row"] = (raw.copy(), raw.shape[0] - 32)
    broken["truncated to the header"] = (raw.copy(), 32)
    broken["shorter than a header"] = (raw.copy(), 16)
    b = raw.copy()
    b[12:16].view(np.int32)[0] = -1
    broken["negative n_exc"] = (b, None)
    cgood = c_pack(lib, K, M.with_rows(K, 1000, range(1, 400)))[0]
    assert cgood.form == M.COLUMNS
    b = cgood.raw.copy()
    b[12:16].view(np.int32)[0] = 1
    broken["rows in the columns form"] = (b, None)
    broken["columns truncated"] = (cgood.raw.copy(), cgood.nbytes - 32)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    fn = lib.fn["decisions_unpack" if K == M.DECISIONS else "proposals_unpack"]
    for name, (b, nbytes) in broken.items():
        nbytes = b.shape[0] if nbytes is None else nbytes
        with pytest.raises(GpxError, match="rc=-1"):
            c_unpack(lib, K, b, nbytes=nbytes)
        with pytest.raises(ValueError):
            M.unpack(K, b[:nbytes])
        outs = [np.full(n, 0x5A5A5A5A, np.int32) for _ in range(5 if K == M.DECISIONS else 4)] + [np.full(n, 0x5A, np.uint8)]
        cnt = ctypes.c_int32(-7)
        assert fn(ptr(b), nbytes, n, *[ptr(c) for c in outs], ctypes.byref(cnt)) == -1, name
        assert cnt.value == -7 and all((c == c[0]).all() for c in outs), f"{name}: partial output"
    same_cols(c_unpack(lib, K, raw), M.unpack(K, raw), "the intact buffer")


def test_packed_out_view_and_sizes(lib):
    """The Python view: header fields, the used bytes, and the bytes the format promises against the plain columns."""
    from gigapaxos_amd._abi import GpxError
    from gigapaxos_amd.packed_out import PackedOut, packed_out_bytes

    G = 3000
    p, _ = c_pack(lib, M.PROPOSALS, M.steady(M.PROPOSALS, G))
    d, _ = c_pack(lib, M.DECISIONS, M.steady(M.DECISIONS, G))
    assert p.nbytes == 32 + 4 * G and d.nbytes == 32 + 8 * G            # against 17 G and 21 G
    assert p.raw.shape[0] == p.nbytes and PackedOut(p.raw.copy(), lib=lib).header() == p.header()
    same_cols(p.unpack(lib=lib), M.steady(M.PROPOSALS, G), "view.unpack")
    for n in (1, 5, 64, 1000, 12345):
        for K in KINDS.values():
            for rows in (0, n // 4, n):
                q, _ = c_pack(lib, K, M.with_rows(K, n, range(n - rows, n)))
                assert q.nbytes <= packed_out_bytes(n) and (q.form == M.COLUMNS or q.nbytes <= 16 * n + 64)
    with pytest.raises(GpxError):
        PackedOut(np.zeros(16, np.uint8), lib=lib)
    with pytest.raises(GpxError):
        PackedOut(p.raw[:64].copy(), lib=lib)                           # the header names more than there is
