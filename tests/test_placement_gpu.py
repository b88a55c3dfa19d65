"""Parity on misaligned columns, odd tails and guarded buffers (tests/placement_common.py).

Every kernel that reads a caller's column with 16-byte loads has a scalar twin for columns that are not 16-byte aligned
and a tail form for the last records of a batch.  The rest of the suite hands the *_dev calls torch allocations
(aligned to 256 bytes, nothing of the test's next to them) and the asynchronous calls whole pages, so those twins and
most tails never ran.  Here every input and output column of a call lies at a chosen offset modulo 16 inside ONE byte
buffer, between guard bands: sentinels around the outputs, live poison - further valid records - around the inputs.

  (a) every fuzz cell of geometry_common.CELLS through PlacedDevEngine, each call under the next of eight placements,
      engine against oracle, the kernels of every call asserted from the launch profile;
  (b) small directed calls at the kernels' own boundaries (8 records per lane, 2,048 / 4,096 per workgroup, the scatter
      tiles' partial last tile), where records 0 and n - 1 belong to groups whose exchange the poison continues;
  (c) the asynchronous host calls with all their columns carved out of one gpx_host_alloc block or one registered
      block of pages (k_copy_out's scalar branch and its m & 3 tail).

test_placement_model.py runs the same arenas oracle against oracle on the CPU, counts the (entry point, placement) pairs
of (a) and shows that the poison is live."""
import ctypes as C

import numpy as np
import pytest

from gigapaxos_amd import C_HASVALUE, Engine
from tests import placement_common as PC
from tests.geometry_common import CELLS, ar_route, geometry, run_cell
from tests.test_backends_gpu import _env

pytestmark = pytest.mark.gpu


def _fast(value, fast):
    return pytest.param(value, marks=pytest.mark.gpu_fast) if value == fast else value


def _moves_int_input(placement, n):
    """Is one of the call's int32 input columns off a 16-byte boundary?"""
    return placement in PC.MOVES_INT_INPUT or (placement == "packed" and n % 4 != 0)


# ---- (a) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [_fast(n, "partition-k3-w4") for n in CELLS])
def test_cell_under_every_placement(hip_lib, oracle_lib, monkeypatch, name):
    c = CELLS[name]
    _env(monkeypatch, c["env"])
    geo = geometry(c["G"], c["kmax"], c.get("shift"))
    _, ef, _ = run_cell(hip_lib, oracle_lib, c, steps=PC.PLACED_STEPS[name], counted=PC.PlacedDevEngine)
    short = {k: v for k, v in PC.cell_counts(ef.log).items() if v < 1}
    assert not short, (name, short)
    scatter = "k_scatter_ac16" if geo["ac16"] else "k_scatter_ac"
    tiled = {p: 0 for p in PC.NAMES}
    for i, x in enumerate(ef.log):
        op, n, p, ran = x["op"], x["n"], x["placement"], x["kernels"]
        what = (name, i, op, n, p, sorted(ran))
        if op in ("accept", "commit"):
            assert scatter in ran, what
        if op == "accept_reply" and name.startswith("tiles-") and n > 1024:
            assert ar_route(geo, n, sar_max_n=0)[0] == "tiles", (name, n)
            if _moves_int_input(p, n):
                assert "k_scatter_ar16" in ran and "k_scatter_tiles" not in ran, what
            else:
                assert "k_scatter_tiles" in ran and "k_scatter_ar16" not in ran, what
                tiled[p] += 1
        if op == "accept_reply" and name.startswith("partition-"):
            assert {"k_hist", "k_scatter_ar16"} <= ran, what
    if name.startswith("tiles-"):
        assert tiled["aligned"] and tiled["only-outputs"], tiled
    if name.startswith("big-"):
        for p in ("all+4", "only-gidx"):
            assert any("k_order_check" in x["kernels"] for x in ef.log if x["placement"] == p and x["op"] in ("accept", "commit")), p


# ---- (b) ------------------------------------------------------------------------------------------------------------------
def _case(hip_lib, oracle_lib, monkeypatch, kind, placement, status_at=None, status=True):
    PC.case_env(monkeypatch, kind)
    _, G, _, sizes, kernels = PC.CASES[kind]
    for n in sizes:
        ea, eb = PC.case_pair(hip_lib, oracle_lib, kind)
        pa = PC.PlacedDevEngine(ea)
        pa.fixed, pa.gmax, pa.status_at, pa.null_status = placement, G - 1, status_at, not status
        PC.drive_case(kind, n, pa, eb)
        data = [x for x in pa.log if x["op"] in kernels]
        assert {x["op"] for x in data} == set(kernels)
        for x in data:
            assert x["n"] == n and kernels[x["op"]] <= x["kernels"], (kind, n, placement, x["op"], sorted(x["kernels"]))
        ea.close(), eb.close()


@pytest.mark.parametrize("placement", ["all+4", "aligned"])
@pytest.mark.parametrize("kind", ["order", "one", "pers", "small", "runs"])
def test_tails_of_the_ordered_kernels(hip_lib, oracle_lib, monkeypatch, kind, placement):
    """order: k_order_check (8 records per lane, 2,048 per workgroup) in front of unpromised grouped ACCEPT / COMMIT
    batches just past the fused launch's 65,536 records.  one / pers / small: k_one_check with k_propose_one / k_ac_one,
    the one-launch forms k_propose_pers / k_ac_pers, and k_ac_small, at 1 .. 2,055 records.  runs: k_runs_check (4,096
    records per workgroup) and k_ar_runs on three ascending runs."""
    _case(hip_lib, oracle_lib, monkeypatch, kind, placement)


@pytest.mark.parametrize("status_at", [_fast(0, 0), 1, 2, 3, None])
def test_tiled_front_end_partial_last_tile(hip_lib, oracle_lib, monkeypatch, status_at):
    """GPX_TILE_T=4096: two full tiles and a partial one of 0, 1, 2, 3 and 5 votes, and one tile of 4,095; columns aligned,
    the status column at +0 .. +3 and NULL.  The partial tile's column loads stand in front of the tile's first barrier:
    the poison behind the columns is what they would bring in."""
    geo = geometry(PC.CASES["tiles"][1], 3)
    for n in PC.TILE_N:
        assert ar_route(geo, n, sar_max_n=0, force_T=4096)[:2] == ("tiles", 4096)
    _case(hip_lib, oracle_lib, monkeypatch, "tiles", "aligned", status_at=status_at or 0, status=status_at is not None)


@pytest.mark.parametrize("placement", ["all+4", "only-gidx"])
def test_partition_front_end_tails(hip_lib, oracle_lib, monkeypatch, placement):
    """GPX_AR_TILES=0, the same sizes: k_hist and k_scatter_ar16 on columns off the 16-byte boundary."""
    _case(hip_lib, oracle_lib, monkeypatch, "partition", placement)


# ---- (c) ------------------------------------------------------------------------------------------------------------------
def _async_columns(op, m, eh, eo):
    """Input columns of one asynchronous call of an odd number of records whose compacted outputs have m entries (the
    per-record outputs: n), after the host calls that prepare both engines for it."""
    G = int(eo.cfg.max_groups)
    every = np.arange(G, dtype=np.int32)
    n = 2 * m + 5
    assert n % 2 == 1 and n <= G
    g = every[:n].copy()
    if op == "propose":
        return [g, np.zeros(n, np.uint8)]
    pa, pb = eh.propose(every), eo.propose(every)
    assert all(x.tolist() == y.tolist() for x, y in zip(pa, pb))
    if op == "accept":
        return [g, pb[1][:n], pb[2][:n], pb[0][:n], pb[3][:n], np.zeros(n, np.uint8)]
    if op == "commit":   # the first m commits carry their value and execute, the others are placeholders
        kind = np.zeros(n, np.uint8)
        kind[:m] = C_HASVALUE
        return [g, pb[1][:n], pb[2][:n], pb[0][:n], pb[3][:n], kind]
    # votes dropped until m groups have their second: groups 0 .. m-1 decide
    gi = np.concatenate([every[:n - m], every[:m]]).astype(np.int32)
    acc = np.concatenate([np.full(n - m, 101), np.full(m, 102)]).astype(np.int32)
    order = np.random.default_rng(m).permutation(n)
    return [gi[order], np.zeros(n, np.int32), np.full(n, 100, np.int32), np.ones(n, np.int32), acc[order], np.zeros(n, np.int32)]


@pytest.mark.parametrize("memory", ["gpx_host_alloc", "registered pages"])
def test_async_calls_on_columns_carved_from_one_block(hip_lib, oracle_lib, memory):
    """The raw *_async entries with every input and output column inside one block, `packed` and `all+4`, n odd, the
    count of compacted entries 0, 1 and 3 modulo 4: k_copy_out's scalar branch and its m & 3 tail.  The bytes around the
    outputs keep their sentinels, the inputs are untouched, the answer is the oracle's."""
    from tests.parity_common import make_pair
    from gigapaxos_amd import hri_create, S_OK
    G = 64
    for op in PC.OPS:
        for placement in ("packed", "all+4", "aligned"):   # (aligned: the 16-byte stores, sentinels right behind them)
            for m in (8, 9, 11):
                eh, eo = make_pair(hip_lib, oracle_lib, 100, G, 3, 8, max_batch=4096)
                for e in (eh, eo):
                    assert (e.create_groups(np.arange(G), np.tile(np.array(PC.MEMBERS, np.int32), (G, 1)), 3,
                                            hri_create(G, 3, 100)) == S_OK).all()
                cols = _async_columns(op, m, eh, eo)
                n = cols[0].shape[0]
                fn, ins, outs = PC.OPS[op]
                front, behind = PC.poison(op, cols)
                columns = [PC.Column(nm, w, n, False, a, f, b) for (nm, w), a, f, b in zip(ins, cols, front, behind)]
                columns += [PC.Column(nm, w, 1 if nm in PC.COUNT_WORDS else n, True) for nm, w in outs]
                image = PC.lay_out(placement, columns)
                if memory == "gpx_host_alloc":
                    block = eh.host_alloc(image.shape[0], np.uint8)
                else:
                    block = Engine.page_array(image.shape[0], np.uint8)
                    eh.host_register(block)
                assert block.ctypes.data % 16 == 0
                block[:] = image
                ptr = [C.c_void_p(block.ctypes.data + c.off) for c in columns]
                if op == "accept_reply":   # (a common ballot goes in between the columns: none here)
                    ptr = ptr[:3] + [0, 0] + ptr[3:]
                t = C.c_uint64(0)
                eh.lib.check(eh.lib.fn[fn + "_async"](eh.h, n, *ptr, C.byref(t)), fn + "_async")
                eh.lib.check(eh.lib.fn["engine_wait"](eh.h, t), "engine_wait")
                after = np.array(block)
                what = f"{op}_async, {placement}, n={n}, m={m}, {memory}"
                PC.verify(image, after, columns, what)
                want = PC.host_call(eo, op, cols)
                key, comp, word = PC.COMPACTED[op]
                got = {c.name: after[c.off:c.off + c.nbytes].view(c.dtype()) for c in columns if c.out}
                if word:
                    assert int(got[word][0]) == int(want[word][0]) == (0 if op == "accept" else m), (what, got[word], want[word])
                for nm, _ in outs:
                    k = 1 if nm in PC.COUNT_WORDS else (int(want[word][0]) if nm in comp else n)
                    assert got[nm][:k].tolist() == want[nm][:k].tolist(), (what, nm)
                assert eh.snapshot(np.arange(G))[0].tobytes() == eo.snapshot(np.arange(G))[0].tobytes(), what
                assert eh.counters() == eo.counters(), what
                if memory == "gpx_host_alloc":
                    eh.host_free(block)
                else:
                    eh.host_unregister(block)
                del block
                eh.close(), eo.close()
