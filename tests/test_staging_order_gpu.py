"""The arrival order, the checkpoints and the slot age of the regular round on the tiled per-bucket accept-reply kernels
(bucket16_body's two-word staging, gigapaxos_amd/csrc/gpx_ar16.hip.h), the HIP engine against the oracle.

The kernel rebuilds the arrival order of a group's votes from a key (tile << 14 | offset in the tile), the rank an LDS
atomic returns and a five-comparator sorting network; the order shows in ONE place, the median_cp of the decision -
getMedianMinus at the vote that completes the majority (PCS:597-640, 859-875) - and only when the votes carry different
checkpoints.  streams.vote_round gives every vote max_cp = slot - 1; the streams here (tests/staging_common.py:
order_round) give every vote its own, so that a dropped comparator, a key without its tile bits or its top offset bit,
or a network that sorts the wrong way round changes decisions.  The cases (staging_common.CASES): one to four tiles,
tiles of 16,384 votes (bit 13 of the offset), 256 / 512 / 1,024 lanes per bucket, groups of one to five, both edges of the
checkpoint byte and of the slot byte and the escapes just past them, older outstanding slots up to the window and past
it, retransmitted votes of a decided slot, a fourth vote (duplicate or stranger) at every rank, two votes, a single vote,
slots across Integer.MAX_VALUE, and the same stream on the four-word layout (a partial bucket, a lower ballot in every
bucket, K = 5).  Compared per call: proposals, decisions in order, per-vote status; at the end every HotRestoreInfo row
and the counters.  tests/test_staging_order_model.py shows on the CPU that every case reaches what it claims: which
buckets are regular, that the order changes decisions, that the tiles and the bytes are reached.  The engine has no
counter for "this bucket took the short path"; profiles/r18_staging_order_tests.txt lists the kernel mutants each case
catches instead."""
import pytest

from tests.staging_common import CASE, CASES, Driver
from tests.test_two_word_staging_gpu import Pair

pytestmark = pytest.mark.gpu


class GpuDriver(Driver):
    def reply(self, cols, what, irregular):
        assert self.route(cols[0].shape[0]) in self.case["tiles"], what  # geometry_common's restatement: tiled, this many tiles
        return self.p.reply(cols, "%s: %s" % (self.case["name"], what))


@pytest.mark.parametrize("name", [pytest.param(c["name"], marks=pytest.mark.gpu_fast) if c["name"] == "order-2048" else c["name"]
                                  for c in CASES])
def test_staging_order(monkeypatch, hip_lib, oracle_lib, name):
    case = CASE[name]
    p = Pair(monkeypatch, hip_lib, oracle_lib, **case["pair"])
    case["script"](GpuDriver(p, case))
    p.finish(kernel=case.get("kernel", "k_bucket_ar16_tiles_k4"))  # k_scatter_tiles and this per-bucket kernel ran
