"""Delta images (include/gpx_delta.h): the numpy model (tests/delta_model.py) against hand-written answers, and the model
driven through the history of tests/test_group_delta_gpu.py's mirror test, oracle against oracle: its changed and gone
sets and its marks against the differences of the dumps, with a call that `cap` and `cap_gone` cut in every round.  The
same run shows that the history is not vacuous: every round changes a part of the table, not all and not nothing;
somewhere a group changes in p_ring's responded mask alone (one vote below majority: one word of the row); groups gain a
continuation row and lose it again."""
import numpy as np
import pytest

from gigapaxos_amd import image
from tests import delta_common as DC
from tests import image_model as IM
from tests.delta_model import DeltaModel, EVICT, FULL


def test_model_hand_written():
    assert (EVICT, FULL) == (image.DELTA_EVICT, image.DELTA_FULL)        # the model's flags are the binding's
    m = DeltaModel(6)
    A, B, C = (1, 5), (1, 6), (1, 7)
    dumps = [A, None, B, A, None, C]
    nrows = [1, 0, 2, 1, 0, 1]
    r = m.export(dumps, nrows)                                           # counts only
    assert r["counts"] == (4, 4, 5, 0, 0, 0, 0, 0) and m.mark == [None] * 6
    r = m.export(dumps, nrows, cap=2)                                    # group 2 needs two rows, one is left
    assert r["written"] == [0] and r["counts"] == (4, 4, 5, 1, 1, 0, 0, 0)
    r = m.export(dumps, nrows, cap=2)                                    # it is reported again; 3 does not fit behind it
    assert r["changed"] == [2, 3, 5] and r["written"] == [2] and r["counts"] == (4, 3, 4, 1, 2, 0, 0, 0)
    r = m.export(dumps, nrows, cap=9, cap_gone=9)
    assert r["written"] == [3, 5] and r["counts"] == (4, 2, 2, 2, 2, 0, 0, 0)
    assert m.export(dumps, nrows, cap=9, cap_gone=9)["counts"] == (4, 0, 0, 0, 0, 0, 0, 0)      # nothing happened
    dumps = [A, None, None, B, C, None]                                  # 2 and 5 died, 3 changed, 4 was created
    r = m.export(dumps, nrows=[1, 0, 0, 1, 1, 0], cap=9, cap_gone=1)
    assert r["written"] == [3, 4] and r["gone"] == [2, 5] and r["listed"] == [2] and r["counts"] == (3, 2, 2, 2, 2, 2, 1, 0)
    r = m.export(dumps, nrows=[1, 0, 0, 1, 1, 0], entries=[5, 9, -1, 0], cap=9, cap_gone=9)   # listed, out of range
    assert r["listed"] == [5] and r["counts"] == (1, 0, 0, 0, 0, 1, 1, 0)
    dumps[5] = C                                                         # created again in the state it had: its mark is gone
    assert m.export(dumps, [1, 0, 0, 1, 1, 1], cap=9)["written"] == [5]
    r = m.export(dumps, [1, 0, 0, 1, 1, 1], entries=[4, 0], flags=FULL | EVICT, cap=1)
    assert r["written"] == [4] and r["counts"] == (2, 2, 2, 1, 1, 0, 0, 0) and m.mark[4] is None and m.mark[0] == A
    dumps[4] = None                                                      # evicted: dead, and not gone
    assert m.export(dumps, [1, 0, 0, 1, 0, 1], cap=9, cap_gone=9)["counts"] == (3, 0, 0, 0, 0, 0, 0, 0)


def rows_of(d, g, shape):
    return IM.row_from_dump(np.asarray(d, np.int32), g, DC.ME, shape["kmax"], shape["window"])


@pytest.mark.parametrize("name", list(DC.SHAPES))
def test_model_over_the_mirror_history(oracle_lib, name):
    assert (EVICT, FULL) == (image.DELTA_EVICT, image.DELTA_FULL)
    shape = DC.SHAPES[name]
    rng = np.random.default_rng(shape["seed"])
    ea, eb = DC.engine(oracle_lib, shape), DC.engine(oracle_lib, shape)
    DC.populate(ea, eb, shape, rng)
    L = image.layout(shape["kmax"], shape["window"])
    dumps = lambda: [tuple(ea.dump(g).tolist()) for g in range(DC.N)]
    before = dumps()
    m = DeltaModel(DC.N)
    r0 = m.export(before, [1] * DC.N, flags=FULL, cap=DC.N)              # the baseline: every group is live and at rest
    assert r0["written"] == list(range(DC.N)) and m.mark == before
    ctx, mask_alone, gained, lost, died, born = {}, 0, 0, 0, 0, 0
    for r in range(DC.ROUNDS):
        DC.mirror_round(ea, eb, shape, rng, r, ctx)
        now = dumps()
        live = [g for g in range(DC.N) if now[g][0]]
        changed = [g for g in live if now[g] != before[g]]
        print(f"{name} round {r}: {len(changed)} of {len(live)} live groups changed")
        assert 0.05 * len(live) <= len(changed) <= 0.60 * len(live), (r, len(changed), len(live))
        # the model: a call that both caps cut, then the rest; together exactly the differences of the dumps
        dl = [d if d[0] else None for d in now]
        nrows = [rows_of(d, g, shape).shape[0] if d else 0 for g, d in enumerate(dl)]
        dead = [g for g in range(DC.N) if before[g][0] and not now[g][0]]
        need = sum(nrows[g] for g in changed)
        r1 = m.export(dl, nrows, cap=need // 2, cap_gone=len(dead) // 2)
        assert r1["changed"] == changed and r1["gone"] == dead and r1["counts"][:3] == (len(live), len(changed), need)
        assert r1["written"] == changed[:len(r1["written"])] and 0 < len(r1["written"]) < len(changed)
        assert r1["listed"] == dead[:len(dead) // 2] and need // 2 - 1 <= r1["counts"][4] <= need // 2
        for g in range(DC.N):                                            # marks move for what was written, and only for that
            want = dl[g] if g in r1["written"] else None if g in r1["listed"] else (before[g] if before[g][0] else None)
            assert m.mark[g] == want, (r, g)
        r2 = m.export(dl, nrows, cap=need, cap_gone=len(dead))
        assert r1["written"] + r2["written"] == changed and r1["listed"] + r2["listed"] == dead
        assert r2["changed"] == r2["written"] and m.mark == dl
        assert m.export(dl, nrows, cap=need, cap_gone=len(dead))["counts"] == (len(live), 0, 0, 0, 0, 0, 0, 0)
        for g in range(DC.N):
            if before[g][0] and not now[g][0]:
                died += 1
            if now[g][0] and not before[g][0]:
                born += 1
        for g in changed:
            if not before[g][0]:
                continue
            a, b = rows_of(before[g], g, shape), rows_of(now[g], g, shape)
            gained += a.shape[0] == 1 and b.shape[0] == 2
            lost += a.shape[0] == 2 and b.shape[0] == 1
            if a.shape == b.shape:
                wa, wb = a.view("<u4").reshape(-1), b.view("<u4").reshape(-1)
                d = np.nonzero(wa != wb)[0]
                if d.size == 1 and L["p"] <= d[0] < L["p"] + shape["window"] and (wa[d[0]] ^ wb[d[0]]) < 0x10000:
                    mask_alone += 1
        before = now
    print(f"{name}: {mask_alone} responded masks alone, {gained} rows gained, {lost} lost, {died} died, {born} born")
    assert mask_alone >= 1 and gained >= 1 and lost >= 1 and died >= 1 and born >= 1
    for g in range(DC.N):
        assert ea.dump(g).tolist() == eb.dump(g).tolist()
    ea.close()
    eb.close()
