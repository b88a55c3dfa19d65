"""The drivers of tests/test_elect_enum_gpu.py over the oracle, on the CPU, with the FULL enumerations - and what keeps
the GPU legs from being vacuous: every outcome at every arrival position that can produce it, every entry kind, the
duplicate-handle drop and its exception below the carried range, a higher ballot replacing a carried pvalue, the order
of the replies mattering, list entries on both sides of Integer.MAX_VALUE, the W = 4 leg refusing where the restated
limits say and nowhere else.

Counts (groups = 6 shapes x letters^L; letters = 6 per member + 5, + 3 extended, + 1 at W = 4):

  K  W   L  alphabet   groups   elected  preempted   refused (clash / span / length)
  3  8   3  base        73,002   45,360    14,844    none      (the issue's prototype: reproduced exactly)
  3  8   3  extended   105,456   68,412    19,008    none
  3  64  3  extended   105,456   68,412    19,008    none
  3  4   3  + sixth    118,098   63,374    21,280    6,588 / 5,586 / 5,796 in 15,634 groups (13.2 %)
  1  8   3  extended    16,464   13,338     2,964    none
  2  8   3  extended    48,000   22,512    11,664    none
  5  8   3  extended   329,232       see COUNTS      none
"""
import numpy as np
import pytest

from tests import elect_enum_common as EC

# (K, W, L, extended) -> (groups, elected, preempted) of the full enumeration, either base
COUNTS = {
    (3, 8, 3, False): (73_002, 45_360, 14_844),
    (3, 8, 3, True): (105_456, 68_412, 19_008),
    (3, 64, 3, True): (105_456, 68_412, 19_008),
    (3, 4, 3, True): (118_098, 63_374, 21_280),
    (1, 8, 3, True): (16_464, 13_338, 2_964),
    (2, 8, 3, True): (48_000, 22_512, 11_664),
}
LEGS = [(3, 8, "plain", "per-step", False), (3, 8, "plain", "one-call", True), (3, 8, "wrap", "per-step", True),
        (3, 64, "plain", "per-step", True), (3, 64, "wrap", "one-call", True), (3, 4, "plain", "one-call", True),
        (1, 8, "plain", "one-call", True), (1, 8, "wrap", "per-step", True), (2, 8, "plain", "per-step", True),
        (2, 8, "wrap", "one-call", True), (3, 8, "wrap+1", "per-step", True)]


def possible(K, pos):
    """The outcomes arrival position pos can produce with K members (majority: more than K / 2 distinct members)."""
    out = {"ignored", "preempted"}
    if K > 1:
        out.add("recorded")
    if pos >= K // 2:
        out.add("elected")
    return out


def not_vacuous(st, K, W, L, base, extended, full=True):
    for pos in range(L):
        seen = {k for k, v in st.kinds[pos].items() if v}
        assert seen >= possible(K, pos), (pos, st.kinds[pos])
        if W >= 8:
            assert seen == possible(K, pos), (pos, st.kinds[pos])
    assert st.entries["carry"] and st.entries["noop"] and st.entries["preactive"], st.entries
    assert st.dup_dropped > 0
    if K > 1:
        assert st.replaced > 0, "a pvalue of a higher ballot never replaced a carried one"
    if extended and W >= 8:
        assert st.entries["newstop"] > 0 and st.dup_kept > 0, (st.entries, st.dup_kept)
    if base == "wrap+1":
        assert st.pre_both_sides > 0, "no list with PRE-ACTIVE proposals on both sides of Integer.MAX_VALUE"
    if base.startswith("wrap"):
        assert st.both_sides * 10 >= st.elected, "list entries on both sides of Integer.MAX_VALUE in a tenth of the elections"
    else:
        assert st.both_sides == 0
    if full:
        share = EC.reversal_share(st, L)
        assert share >= 0.1, f"reversing the replies changes the outcome of {share:.1%} of the groups"
    # conditions, not measurements
    if W >= 8:
        assert sum(st.refused.values()) == 0 and st.groups_refused == 0, st.refused
    else:
        assert all(st.refused.values()), st.refused
        assert 0.1 <= st.groups_refused / st.groups <= 0.5, (st.groups_refused, st.groups)
        assert st.after_refusal > 0, "no refused group was elected or preempted by a later reply"


@pytest.mark.parametrize("K,W,base,form,extended", LEGS, ids=[f"{K}-{W}-{b}-{f}-{'ext' if x else 'base'}" for K, W, b, f, x in LEGS])
def test_enumeration_on_the_oracle(oracle_lib, K, W, base, form, extended):
    st = EC.run_enum(oracle_lib, K, W, 3, base, form, extended=extended, flip=base == "wrap")
    assert (st.groups, st.elected, st.preempted) == COUNTS[(K, W, 3, extended)], st.summary()
    not_vacuous(st, K, W, 3, base, extended)


def test_five_members_full(oracle_lib):
    st = EC.run_enum(oracle_lib, 5, 8, 3, "plain", "one-call")
    assert st.groups == 6 * 38 ** 3
    print(st.summary())
    # (no reversal condition here: with five members three replies elect only when all three count, and then carry
    # over the same set of pvalues in either order - but for the two letters that name slot S0 + 3 in one ballot as two
    # requests, of which the first to arrive stays: 0.7 % of the groups; a preemption hands over the same pre-actives
    # wherever it stands.  The order of the replies matters from the fourth on - test_sampled_legs - and with fewer members)
    not_vacuous(st, 5, 8, 3, "plain", True, full=False)
    assert 0.0 < EC.reversal_share(st, 3) < 0.02


@pytest.mark.parametrize("K,L,base", [(5, 3, "wrap"), (3, 4, "plain"), (3, 4, "wrap")])
def test_sampled_legs(oracle_lib, K, L, base):
    """The GPU file's samples of 60,000: K = 5 across the wrap, and four replies - the fourth meets a coordinator that is
    active already, or gone."""
    from tests.test_elect_enum_gpu import SAMPLE_60K
    st = EC.run_enum(oracle_lib, K, 8, L, base, "one-call", sample=SAMPLE_60K, flip=base == "wrap")
    assert st.groups == 60_000
    not_vacuous(st, K, 8, L, base, True, full=False)
    if L == 4:
        assert st.kinds[3]["ignored"] > st.groups // 2 and st.kinds[3]["elected"] > 0 and st.kinds[3]["preempted"] > 0


def test_gpu_samples_are_not_vacuous(oracle_lib):
    """The sample of 16,000 the GPU legs with three members take, at every window."""
    from tests.test_elect_enum_gpu import SAMPLE
    for W, base in ((8, "wrap"), (4, "plain"), (64, "plain")):
        st = EC.run_enum(oracle_lib, 3, W, 3, base, "one-call", sample=SAMPLE)
        not_vacuous(st, 3, W, 3, base, True, full=False)


def test_layouts():
    for G in (1, 4, 5, 6, 1001):
        for L in (3, 4):
            assert EC.check_layout(EC.layout(G, L, "per-step"), G, L)[0] >= 0 or G == 1
            EC.check_layout(EC.layout(G, L, "one-call"), G, L)
    lo, hi = EC.check_layout(EC.layout(16_000, 3, "one-call"), 16_000, 3)
    assert 1 <= lo <= EC.NEAR and hi > EC.scatter_tile(), (lo, hi)   # a few entries apart; in another scatter tile
    a, b = EC.layout(1001, 3, "one-call")[0], EC.layout(1001, 3, "one-call", flip=True)[0]
    assert a[0][0] != b[0][0] and sorted(a[0].tolist()) == sorted(b[0].tolist())


@pytest.mark.parametrize("base", ["plain", "wrap"])
def test_sixteen_members(oracle_lib, base):
    st = EC.run_sixteen(oracle_lib, base=base)
    assert st.elected == st.groups == 48


def test_engine_refusal_by_hand():
    """The three refusals and their neighbours, W = 4, three members, slots around 5."""
    I, C_ = EC.I32, EC.Candidate
    b = (0, 7)

    def cand(heard=(), carry=(), ns=(-1, -1, -1), pre=0):
        c = C_(3, (2, 101), I(5))
        for i in range(pre):
            c.propose(9001 + i)
        c.heard = [j in heard for j in range(3)]
        c.carry = {I(s_): (b, 50 + s_, False) for s_ in carry}
        c.node_slots = [v if v == -1 else I(v) for v in ns]
        return c
    pv = lambda *slots: [(I(s_), b, 50 + s_, False) for s_ in slots]   # noqa: E731
    assert EC.engine_refusal(cand(), (0, I(5), pv(4, 8)), 4) == "clash"                 # inside one reply
    assert EC.engine_refusal(cand(), (0, I(5), pv(4, 7)), 4) is None
    assert EC.engine_refusal(cand({0}, [4], (4, -1, -1)), (1, I(5), pv(8)), 4) == "clash"   # against what is carried
    assert EC.engine_refusal(cand({0}, [4], (4, -1, -1)), (1, I(5), pv(4)), 4) is None      # the same slot again
    assert EC.engine_refusal(cand({0}, [], (4, -1, -1)), (1, I(4), pv(8)), 4) == "span"     # 4 .. 8: five slots
    assert EC.engine_refusal(cand({0}, [], (5, -1, -1)), (1, I(5), pv(8)), 4) is None       # 5 .. 8: four
    assert EC.engine_refusal(cand((), [], (-1, -1, -1)), (1, I(4), pv(8)), 4) is None       # no majority yet
    assert EC.engine_refusal(cand({0}, [], (4, -1, -1), pre=3), (1, I(5), pv(4)), 4) is None    # range 5 .. 4 empty: 5, 6, 7 again
    assert EC.engine_refusal(cand({0}, [], (8, -1, -1), pre=3), (1, I(8), pv(9)), 4) == "length"  # 8, 9 + three again
    assert EC.engine_refusal(cand({0}, [], (8, -1, -1), pre=2), (1, I(8), pv(9)), 4) is None
    # exactly 2^31 apart: the unheard members' -1 against slot Integer.MAX_VALUE
    c = cand({0}, [], (-1, -1, -1))
    c.node_slots = [-1, -1, -1]
    assert EC.engine_refusal(c, (1, I(-1), [(I(2 ** 31 - 1), b, 1, False)]), 8) == "span"


def test_device_branch_driver_on_the_oracle(oracle_lib):
    """test_elect_enum_gpu.test_device_only_branches' driver with the oracle's host call behind include/gpx.h's sentence
    about unvalidated offsets (HostAsElectDev): the batches are what they claim to be."""
    seen, _ = EC.run_device_branches(oracle_lib, oracle_lib, dev=False)
    assert seen["last slice ends at pv_total"] >= 100 and seen["last slice ends at pv_total + 1"] == seen["last slice ends at pv_total"] + 1
    assert np.isin(["n = 1", "n = 4095", "n = 4096", "n = 4097"], list(seen)).all()
