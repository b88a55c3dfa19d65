"""The paxosID table under attack (tests/names_model.py), engine against oracle: collision families of 64 - 256 names
in one probe chain each, families that differ only past the table entry's first 16 bytes, a chain through the last
bucket that wraps to bucket 0, tombstones in the middle of chains, rebuilds, GPX_S_EXISTS, refused lengths, and the
table's copies of (exists, version) after groups are retired or re-created while their names stay bound.  Every
status, row, frame byte and counter equals the oracle's, every lookup the expected row, on both decode tilings."""
import pytest

from tests import names_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["512-frame tiles", "256-frame tiles"])
def _decode_path(request, monkeypatch):
    monkeypatch.setenv("GPX_WD_TILE", "256" if request.param.startswith("256") else "512")


@pytest.mark.parametrize("G", [3000, (1 << 20) + 1])
def test_names_table_under_attack_vs_oracle(hip_lib, oracle_lib, G):
    oh, want, rebuilds, ran = M.names_scenario(hip_lib, G, seed=G, profile=True)
    oo, _, _, _ = M.names_scenario(oracle_lib, G, seed=G)
    assert [s for s, _ in oh] == [s for s, _ in oo]
    for (step, a), (_, b) in zip(oh, oo):
        assert a == b, step
    got = dict(oh)
    for step, w in want.items():
        assert got[step + " lookup" if step + " lookup" in got else step] == w, step
    assert rebuilds == [False, True]
    need = {"k_names_bind", "k_names_unbind", "k_names_lookup", "k_names_coordinator", "k_names_reinsert",
            "k_group_create", "k_group_retire", "k_bucket_pack_ar", "k_emit_frames", "k_pack_scan", "k_pack_write"}
    assert need <= ran, sorted(need - ran)
    assert any(k.startswith("k_wire_decode") for k in ran), sorted(ran)
