"""tests/names_model.py on the CPU: the attack names do what they claim under both hash implementations, and the
scenario of tests/test_names_gpu.py, run on the oracle, meets the lookups and statuses it expects (so that the
engine-against-oracle comparison on the GPU is not vacuous)."""
import ctypes as C

import numpy as np
import pytest

from gigapaxos_amd import S_OK, S_EXISTS, S_NOGROUP
from gigapaxos_amd import wire as W
from tests import names_model as M

BIG_G = (1 << 20) + 1


def _orc_hash(oracle_lib, b):
    f = oracle_lib.lib.orc_java_string_hash
    f.argtypes = [C.c_char_p, C.c_int32]
    f.restype = C.c_int
    return f(b, len(b))


def test_table_geometry():
    assert M.table_geometry(1) == dict(cap=1024, buckets=256, rebuild_after=64)
    assert M.table_geometry(256)["cap"] == 1024 and M.table_geometry(257)["cap"] == 2048
    assert M.table_geometry(3000) == dict(cap=16384, buckets=4096, rebuild_after=1024)
    assert M.table_geometry(BIG_G) == dict(cap=1 << 23, buckets=1 << 21, rebuild_after=1 << 19)


def test_java_hash_rows_matches_the_scalar_hash():
    rng = np.random.default_rng(5)
    rows = rng.integers(0, 256, (500, 23)).astype(np.uint8)
    assert M.java_hash_rows(rows).astype(np.int64).tolist() == [W.java_string_hash(bytes(r)) & 0xFFFFFFFF for r in rows]


@pytest.mark.parametrize("label", sorted(M.families()) + ["wrap-family"])
def test_every_family_collides(oracle_lib, label):
    fam = M.wrap_family(3000) if label == "wrap-family" else M.families()[label]
    assert 64 <= len(fam) <= 256 and len(set(fam)) == len(fam)
    assert len({len(x) for x in fam}) == 1 and 1 <= len(fam[0]) <= 127
    assert len({W.java_string_hash(x) for x in fam}) == 1
    assert len({_orc_hash(oracle_lib, x) for x in fam}) == 1
    assert _orc_hash(oracle_lib, fam[0]) == W.java_string_hash(fam[0])
    if label.endswith("tail") or label == "tail-only":
        assert len({x[:16] for x in fam}) == 1, "members differ only past the table entry's 16 bytes"
    assert len({M.home_bucket(x, 3000) for x in fam}) == 1


def test_family_lengths():
    lens = {len(f[0]) for f in M.families().values()}
    assert {15, 16, 17, 126, 127} <= lens
    assert any(b"\x80" <= bytes([c]) for c in M.families()["len16-high"][0])


@pytest.mark.parametrize("G", [3000, BIG_G])
def test_wrap_names_land_on_the_last_bucket(oracle_lib, G):
    last = M.table_geometry(G)["buckets"] - 1
    names = M.wrap_names(G, 12)
    assert len(set(names)) == 12
    assert all(M.home_bucket(x, G) == last for x in names)
    assert len({W.java_string_hash(x) for x in names}) == 12, "distinct hashes: a chain of the bucket, not a family"
    assert all(_orc_hash(oracle_lib, x) == W.java_string_hash(x) for x in names)
    fam = M.wrap_family(G)
    assert M.home_bucket(fam[0], G) == last


@pytest.mark.parametrize("G", [3000, BIG_G])
def test_names_scenario_on_the_oracle(oracle_lib, G):
    out, want, rebuilds, _ = M.names_scenario(oracle_lib, G, seed=G)
    got = dict(out)
    for step, w in want.items():
        key = step + " lookup" if step + " lookup" in got else step
        assert got[key] == w, step
    assert want["exists"] == [S_EXISTS] * 4 + [S_OK] * 2 and want["refused lengths"] == [S_NOGROUP] * 2
    assert rebuilds == [False, True]
    assert all(s == S_OK for s in got["families"])
    # the decode reaches every bound member (OK), the stale versions (VERSION) and the unbound siblings (NOGROUP)
    st = np.array(got["decode families"][0])
    assert {W.W_OK, W.W_VERSION, W.W_NOGROUP} <= set(st.tolist())
    for tag in ("copies", "copies after rebuild"):
        st = np.array(got[tag + " decode"][0])
        n = st.shape[0] // 2
        k = n // 3
        assert (st[:k] == W.W_NOGROUP).all() and (st[n:n + k] == W.W_NOGROUP).all(), "killed: no group"
        assert (st[2 * k:n] == W.W_OK).all() and (st[n + 2 * k:] == W.W_VERSION).all(), "re-created: new version only"
        assert (np.array(got[tag + " decode restored"][0][:n])[:2 * k] != W.W_NOGROUP).any()
        assert got[tag + " pack_commits"][1], "commits packed for the live groups"
        assert any(u == 1 for u in got[tag + " pack_accept_replies"][3]), "replies of retired groups stay unbatched"
