"""gpx_wire_pack_accepts_dev / gpx_wire_request_sizes_dev without a GPU: declared, exported, bound, and the test
suite's own restatement of latchToBatch + makeAcceptFrame (tests/wire_accepts_model.py) checked against the frame
builders and the Java reading of tests/wire_model.py."""
import ctypes
import os
import re
import struct

import numpy as np

from gigapaxos_amd import wire as W
from tests import wire_model as JM
from tests import wire_accepts_model as AM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gpx_wire_request_sizes_dev", "gpx_wire_pack_accepts_dev")


def test_both_symbols_declared_and_exported():
    import __graft_entry__ as ge

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpx_wire.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
    ge.build()
    lib = ctypes.CDLL(ge.HIP_SO)
    for name in NEW:
        assert hasattr(lib, name), name


def test_wire_binding_loads_them():
    import __graft_entry__ as ge
    from gigapaxos_amd import load_hip

    ge.build()
    for name in NEW:
        assert name[4:] in W.WIRE_EXPORTED_SYMBOLS
    lib = W.bind_wire(load_hip())
    for name in NEW:
        assert name[4:] in lib.fn
    assert callable(W.pack_accepts_dev) and callable(W.request_sizes_dev)


def _fields(rng, name, rid):
    value = bytes(rng.integers(0, 256, int(rng.integers(0, 300))).astype(np.uint8))
    return dict(paxos_id=name, version=int(rng.integers(0, 3)), req_id=rid, value=value, stop=bool(rng.random() < 0.1))


def test_restatement_agrees_with_builders_and_java_reading():
    rng = np.random.default_rng(5)
    for it in range(300):
        name = bytes(rng.integers(0x21, 0x7f, int(rng.integers(1, 128))).astype(np.uint8))
        k = int(rng.integers(1, 6))
        heads = [_fields(rng, name, (it << 8) + q) for q in range(k)]
        own = [[W.request(name, h["version"], h["req_id"] * 10 + j, b"x" * int(rng.integers(0, 9)))
                for j in range(int(rng.integers(0, 3)))] for h in heads]
        reqs = [W.request(h["paxos_id"], h["version"], h["req_id"], h["value"], h["stop"], batched=o)
                for h, o in zip(heads, own)]
        slot, bnum, bcoord, med, sender = (int(x) for x in rng.integers(-2**31, 2**31, 5))
        if k == 1:
            acc = AM.make_accept(reqs[0], slot, bnum, bcoord, med, sender)
            want = W.accept(name, heads[0]["version"], heads[0]["req_id"], slot, bnum, bcoord, med, sender,
                            heads[0]["value"], heads[0]["stop"], batched=own[0])
        else:
            acc = AM.make_accept(AM.latch_to_batch(reqs[0], reqs[1:]), slot, bnum, bcoord, med, sender)
            flat = list(own[0])
            for h, o in zip(heads[1:], own[1:]):
                flat.append(W.request(name, h["version"], h["req_id"], h["value"], h["stop"]))
                flat += o
            want = W.accept(name, heads[0]["version"], heads[0]["req_id"], slot, bnum, bcoord, med, sender,
                            heads[0]["value"], heads[0]["stop"], batched=flat)
        assert acc == want, it
        st, t, p = JM.to_paxos_packet(acc)
        assert st == W.W_OK and t == W.WT_ACCEPT
        assert (p.slot, p.ballot, p.median, p.sender, p.request_id) == (slot, (bnum, bcoord), med, sender,
                                                                        heads[0]["req_id"])
        assert len(p.batched or ()) == (sum(len(o) for o in own) + k - 1)
        assert JM.is_stop_request(p) == any(h["stop"] for h in heads)


def test_restatement_drops_trailing_bytes_and_unparsable_members():
    rng = np.random.default_rng(6)
    a = W.request(b"g", 0, 1, b"abc", batched=[W.request(b"g", 0, 2, b"d")]) + b"\x01\x02\x03"
    b = W.request(b"g", 0, 3, b"e") + b"\xff"
    flat = AM.latch_to_batch(a, [b])
    assert flat == W.request(b"g", 0, 1, b"abc", batched=[W.request(b"g", 0, 2, b"d"), W.request(b"g", 0, 3, b"e")])
    # b_count == 1: the frame verbatim, trailing bytes included
    acc = AM.expected_accepts([a], [0], [0], [1], [5], [6], [7], [8], [0], 100)[0]
    assert acc == AM.make_accept(a, 5, 6, 7, 8, 100) and acc[4:8] == struct.pack(">i", W.WT_ACCEPT)
    bad = b[:20]
    got = AM.expected_accepts([a, bad], [0, 0], [0], [2], [5], [6], [7], [8], [0], 100)
    assert got == [None]
    assert AM.random_request(rng, b"n", 0, 1) is not None
