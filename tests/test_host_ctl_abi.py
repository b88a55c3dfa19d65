"""The control-plane host-pointer calls without a GPU: tests/host_ctl_emulation.cpp compiles the host text as it is
(gpx_ctl_args.inc, gpx_host_stage.inc, the four *_host.inc, gpx_group_host.inc) over stand-ins for the runtime and the *_dev twins, under
AddressSanitizer and UBSan, and runs the twenty entry points at n = 0, 1, 1,001, 3,001 (2^18 + 1 for the lifecycle calls)
on a fresh engine, an engine whose arena fits and one whose arena is too small, with optional pointers there and not, and
with every kind of faulty argument.  Its transcript must be that of the text these calls had before they were staged
through one helper (tests/golden/host_ctl_transcript.txt, made by the same program from that text, which
scripts/host_ctl_previous_text.sh takes out of the history): every return code
and every output byte.  Then every allocation, copy and synchronisation of every call fails in turn."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "host_ctl_transcript.txt")
ENTRY_POINTS = {
    "names_bind", "names_unbind", "names_lookup", "names_coordinator", "election_scan", "gap_scan", "prepare_batch",
    "request_batch", "wire_decode", "pack_accept_replies", "pack_commits", "election_begin", "poke_scan",
    "prepare_reply_batch", "election_scan_hits", "poke_scan_hits", "gap_scan_hits", "pause_sweep", "group_create",
    "group_retire", "group_snapshot"}       # retire and snapshot are the two faces of one of the twenty
COUNTERS = ("allocs", "memsets", "copies", "launches", "syncs")


def parse(text):
    """{(name, variant, bad, n, occurrence): (rc, digest, {counter: value})} in transcript order"""
    calls, seen = {}, {}
    for line in text.splitlines():
        t = line.split()
        if t[0] == "faults:":
            continue
        assert t[1::2][:5] == ["variant", "bad", "n", "rc", "digest"], line
        key = (t[0], int(t[2]), int(t[4]), int(t[6]))
        seen[key] = seen.get(key, 0) + 1
        calls[key + (seen[key],)] = (int(t[8]), t[10], dict(zip(t[11::2], map(int, t[12::2]))))
    return calls


@pytest.fixture(scope="module")
def transcript(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("host_ctl") / "host_ctl_emulation")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "gigapaxos_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "host_ctl_emulation.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout


def test_every_return_code_and_output_byte_is_the_earlier_text_s(transcript):
    new, old = parse(transcript), parse(open(GOLDEN).read())
    assert list(new) == list(old) and len(new) == 449
    assert {k[0] for k in new} == ENTRY_POINTS
    for key, (rc, digest, _) in new.items():
        assert (rc, digest) == old[key][:2], key
    # what the script is made of: sizes, absent optional pointers, faulty arguments, the lifecycle calls' second chunk
    assert {0, 1, 1001, 3001, 5000, (1 << 18) + 1} == {k[3] for k in new}
    for name in ENTRY_POINTS:
        mine = [k for k in new if k[0] == name]
        assert {0, 1, 1001, 3001} <= {k[3] for k in mine if k[2] == 0 and new[k][0] == 0}, name
        assert any(k[1] & 1 for k in mine) and sum(1 for k in mine if k[2]) >= 3, name
        assert all(new[k][0] < 0 for k in mine if k[2]), name
    assert all(new[(name, v, 0, (1 << 18) + 1, 1)][0] == 0 for name in ("group_create", "group_retire", "group_snapshot")
               for v in (0, 1))


def test_no_call_makes_more_runtime_calls(transcript):
    """A call that succeeds allocates, fills, copies, launches and waits no more often than before.  A call that is
    refused after work was queued now waits once for it before the arena goes to the next call: one synchronisation
    more, nothing else."""
    new, old = parse(transcript), parse(open(GOLDEN).read())
    for key, (rc, _, counts) in new.items():
        for c in COUNTERS:
            extra = 1 if rc < 0 and c == "syncs" and counts["memsets"] + counts["copies"] + counts["launches"] else 0
            assert counts[c] <= old[key][2][c] + extra, (key, c)
    # the arena: the first call of an engine takes every buffer from the allocator, the second none but the arena itself,
    # the larger third one what the arena has no room for
    for name in ENTRY_POINTS - {"group_create", "group_retire", "group_snapshot"}:
        first, second, third = (new[(name, 0, 0, 1001, 1)][2], new[(name, 0, 0, 1001, 2)][2], new[(name, 0, 0, 3001, 1)][2])
        assert 2 <= first["allocs"] <= first["memsets"] and second["allocs"] == 1, name   # (unbind also clears its table)
        assert 1 <= third["allocs"] <= third["memsets"], name
    for name, bufs in (("group_create", 5), ("group_retire", 3), ("group_snapshot", 3)):
        for n in (1001, (1 << 18) + 1):                      # once per call, whatever the number of chunks
            assert new[(name, 0, 0, n, 1)][2]["allocs"] == bufs and new[(name, 0, 0, n, 1)][2]["memsets"] == 0
        assert new[(name, 0, 0, (1 << 18) + 1, 1)][2]["syncs"] == 2 == new[(name, 0, 0, (1 << 18) + 1, 1)][2]["launches"]


def test_every_failed_allocation_copy_and_wait_is_reported_and_cleaned_up(transcript):
    """The program itself checks each injection (the call returns an error, the count of live device blocks is what it
    was, nothing is queued behind the last synchronisation, the arena is released) and stops at the first that fails."""
    last = transcript.strip().splitlines()[-1].split()
    assert last[:2] == ["faults:", "ok,"] and int(last[2]) > 800
