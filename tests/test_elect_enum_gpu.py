"""The prepare-reply phase on the GPU, enumerated against the Java reading (tests/elect_enum_common.py): every output of
every reply of every group against round_model.Candidate and the restated engine limits - through the host call step by
step, through ONE host call with the groups interleaved two ways, through the device-pointer call; at windows 4, 8 and
64, with 1, 2, 3, 5 and 16 members, around slot 5 and across Integer.MAX_VALUE; then what only a device-pointer caller
can hand over, the outputs placed between guard bands, and an engine whose call epoch wraps.

The CPU twin (test_elect_enum_model.py) runs the same drivers over the oracle with the full enumerations and asserts
what keeps these legs from being vacuous.  The GPU legs take seeded samples of the enumerations (SAMPLE: the reading is
walked in Python, a few seconds per 50,000 groups; the alphabets are whole).

Proposed for gpu_fast (tests/conftest.py's GPU_FAST), a few seconds together:
  test_elect_enum_gpu.py::test_enumeration[3-64-3-wrap-dev]      bit 63 of the ring masks, the wrap, the device form
  test_elect_enum_gpu.py::test_device_only_branches              the slice check, NULL columns, the memsets"""
import numpy as np
import pytest

from tests import elect_enum_common as EC
from tests import placement_common as PC

pytestmark = pytest.mark.gpu

SAMPLE = (16_000, 2301)      # (groups, seed) of the legs with three members
SAMPLE_60K = (60_000, 2302)  # K = 5 and L = 4
FORMS3 = ("per-step", "one-call", "dev")
LEGS = [(3, W, 3, base, form, SAMPLE) for W in (8, 64) for base in ("plain", "wrap") for form in FORMS3]
LEGS += [(3, 4, 3, "plain", "one-call", SAMPLE), (3, 8, 3, "wrap+1", "one-call", SAMPLE), (3, 64, 3, "wrap+1", "dev", SAMPLE)]
LEGS += [(K, 8, 3, base, "one-call", SAMPLE) for K in (1, 2) for base in ("plain", "wrap")]
LEGS += [(5, 8, 3, base, "one-call", SAMPLE_60K) for base in ("plain", "wrap")]
LEGS += [(3, 8, 4, base, "one-call", SAMPLE_60K) for base in ("plain", "wrap")]


def report(what, st, seconds=None):
    print(f"{what}: {st.groups} groups, {st.records} replies, elected {st.elected}, preempted {st.preempted}, refused "
          f"{st.refused}, kernels {sorted(st.kernels or {})}")


@pytest.mark.parametrize("K,W,L,base,form,sample", LEGS, ids=[f"{K}-{W}-{L}-{b}-{f}" for K, W, L, b, f, _ in LEGS])
def test_enumeration(hip_lib, K, W, L, base, form, sample):
    st = EC.run_enum(hip_lib, K, W, L, base, form, sample=sample, flip=base == "wrap", profile=True)
    report(f"K={K} W={W} L={L} {base} {form}", st)
    assert st.kernels.get("k_bucket_prepare_reply", 0) >= (L if form == "per-step" else 1), sorted(st.kernels)
    assert "k_election_begin" in st.kernels
    assert st.elected > 0 and st.preempted > 0
    if W >= 8:
        assert sum(st.refused.values()) == 0, st.refused          # a condition (the reading alone stays inside W >= 8)
    else:
        assert all(st.refused.values()) and st.after_refusal > 0, (st.refused, st.after_refusal)


@pytest.mark.parametrize("base", ["plain", "wrap"])
@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_sixteen_members_majority_at_the_ninth(hip_lib, base, dev):
    st = EC.run_sixteen(hip_lib, base=base, dev=dev)
    assert st.elected == st.groups


PLACED_SAMPLE = (8_000, 2303)


@pytest.mark.parametrize("placement", PC.NAMES)
@pytest.mark.parametrize("W", [8, 64])
def test_enumeration_on_placed_columns(hip_lib, W, placement):
    """The device form with every input column and each of the eight outputs - the four [W][n] planes among them - at
    the placement's offset inside one arena between guard bands (placement_common.ElectPlacer): nothing outside the
    outputs changes, and planes j >= e_count[i] keep their sentinels."""
    def placed(e):
        p = PC.PlacedDevEngine(e)
        p.fixed = placement
        return p
    st = EC.run_enum(hip_lib, 3, W, 3, "wrap" if W == 64 else "plain", "dev", sample=PLACED_SAMPLE, driver=placed)
    assert [(x["op"], x["placement"]) for x in st.driver.log] == [("election_begin", placement), ("prepare_reply", placement)]
    assert "k_bucket_prepare_reply" in st.driver.log[1]["kernels"] and "k_election_begin" in st.driver.log[0]["kernels"]
    assert st.elected > 0 and st.preempted > 0 and sum(st.refused.values()) == 0


def test_enumeration_across_the_epoch_wrap(hip_lib, monkeypatch):
    """GPX_TEST_EPOCH_WRAP=5: the enumeration step by step on one engine, fresh groups each time, until the call epoch
    has wrapped at least twice.  Every prepare-reply call opens a call epoch (so does every proposal batch between
    them: the prepare-reply calls alone are counted, a lower bound)."""
    from tests import lifetime_common as LC
    wrap, G = 5, 4_000
    LC.assert_switch_is_read(monkeypatch, hip_lib, "GPX_TEST_EPOCH_WRAP")
    monkeypatch.setenv("GPX_TEST_EPOCH_WRAP", str(wrap))
    reps = next(r for r in range(1, 100) if LC.wraps(3 * r, wrap) >= 2)
    e = EC.make_engine(hip_lib, 3, 8, reps * G, EC.BASES["plain"], 3 * G + 64)
    e.profile(2)
    try:
        for r in range(reps):
            st = EC.run_enum(hip_lib, 3, 8, 3, "plain", "per-step", sample=(G, 2310 + r), engine=e,
                             groups=np.arange(r * G, (r + 1) * G, dtype=np.int32))
            assert st.elected > 0 and st.preempted > 0
        prof = {k: v[0] for k, v in e.profile_read().items()}
    finally:
        e.close()
    assert prof["k_bucket_prepare_reply"] == 3 * reps and LC.wraps(prof["k_bucket_prepare_reply"], wrap) >= 2, prof


def test_device_only_branches(hip_lib, oracle_lib):
    seen, launches = EC.run_device_branches(hip_lib, oracle_lib, dev=True)
    print(seen, launches)
    assert seen["last slice ends at pv_total"] >= 100 and seen["last slice ends at pv_total + 1"] == seen["last slice ends at pv_total"] + 1
    assert launches.get("k_bucket_prepare_reply", 0) >= 13, launches
