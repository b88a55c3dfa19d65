"""The paxosID table of the wire codec, restated, and names that attack it.  Test infrastructure only.

Placement (gpx_wire_dev.inc, wire_names_init; gpx_wire.hip.h:12-30, names_find / k_names_bind):
  cap      = the smallest power of two >= 4 G, and at least 1,024 (table entries)
  buckets  = cap / 4 (128-byte buckets of four ways)
  home     = fmix32(String.hashCode) & (buckets - 1); a probe walks bucket by bucket from there and wraps to bucket 0.
Unbinds leave tombstones; gpx_names_unbind rebuilds the table (k_names_reinsert) once the unbind requests since the
last rebuild exceed cap / 16 (gpx_names_unbind, gpx_wire_host.inc).

Names: collision families (2^k names of one String.hashCode: blocks "Aa" / "BB" or a high-byte pair, which agree on
hashCode, so all members share a home bucket whatever the placement), families behind a common prefix of >= 16 bytes
(the table entry's first 16 bytes agree, only the tail compare in the row tells them apart), and names found by a
vectorised counter search whose home is the LAST bucket (their probe chains wrap to bucket 0).

names_scenario() is the GPU scenario of tests/test_names_gpu.py; tests/test_names_model.py runs it oracle against
oracle on the CPU and checks that its lookups are the expected ones, so the GPU comparison is not vacuous."""
import functools
import itertools

import numpy as np

from gigapaxos_amd import Engine, hri_create, streams, S_OK, S_EXISTS, S_NOGROUP, RETIRE_KILL, RETIRE_PAUSE, D_DECISION
from gigapaxos_amd import wire as W
from gigapaxos_amd._abi import Decisions

PAIRS = {"ascii": (b"Aa", b"BB"), "high": (b"\xc1\x9f", b"\xc2\x80")}
MAX_NAME = 127


def table_geometry(G):
    cap = 1024
    while cap < 4 * G:
        cap <<= 1
    return dict(cap=cap, buckets=cap // 4, rebuild_after=cap // 16)


def home_bucket(name, G):
    h = W.java_string_hash(name) & 0xFFFFFFFF
    return int(streams.fmix32(np.array([h], np.uint32))[0]) & (table_geometry(G)["buckets"] - 1)


def java_hash_rows(rows):
    """String.hashCode of each row of a [n, L] uint8 array, as uint32 (vectorised)."""
    rows = np.asarray(rows, np.uint8)
    h = np.zeros(rows.shape[0], np.uint64)
    for c in range(rows.shape[1]):
        h = (h * np.uint64(31) + rows[:, c].astype(np.uint64)) & np.uint64(0xFFFFFFFF)
    return h.astype(np.uint32)


def family(k, prefix=b"", suffix=b"", pairs=("ascii",), fixed=0):
    """2^k names of one String.hashCode: prefix + k varying blocks + `fixed` blocks of the first pair + suffix.
    `pairs` cycles over the blocks (a block of the "high" pair holds bytes >= 0x80)."""
    out = []
    for choice in itertools.product((0, 1), repeat=k):
        body = b"".join(PAIRS[pairs[i % len(pairs)]][c] for i, c in enumerate(choice))
        out.append(prefix + body + PAIRS[pairs[0]][0] * fixed + suffix)
    assert all(len(x) <= MAX_NAME for x in out)
    return out


def families():
    """{label: names}: 64 - 256 names each, of lengths 15, 16, 17, 28, 126 and 127."""
    return {
        "len15": family(7, prefix=b"f"),                                        # 128
        "len16-high": family(8, pairs=("high",)),                               # 256
        "len17": family(8, prefix=b"q"),                                        # 256: differ in the first 16 bytes
        "tail-only": family(6, prefix=b"tenant/0000/svc/"),                     # 64, length 28: differ past byte 16
        "len126-tail": family(6, prefix=b"T" * 16, fixed=49, pairs=("ascii", "high")),   # 64
        "len127-tail": family(7, prefix=b"U" * 17, fixed=48),                  # 128, length 17 + 14 + 96
    }


@functools.lru_cache(maxsize=None)
def wrap_names(G, count, prefix=b"wrap/", digits=8, suffix=b""):
    """`count` names prefix + a decimal counter + suffix whose home is the last bucket (vectorised search)."""
    bm = table_geometry(G)["buckets"] - 1
    M32 = 1 << 32
    ls = len(suffix)
    hp, hs = W.java_string_hash(prefix) % M32, W.java_string_hash(suffix) % M32
    base = np.uint64(hp * pow(31, digits + ls, M32) % M32)
    mul = np.uint64(pow(31, ls, M32))
    pw = np.array([31 ** (digits - 1 - d) for d in range(digits)], np.int64)
    found = []
    lo = 0
    chunk = min(1 << 22, 4 * (bm + 1) * count)
    while len(found) < count:
        c = np.arange(lo, lo + chunk, dtype=np.int64)
        dig = (c[:, None] // (10 ** np.arange(digits - 1, -1, -1, dtype=np.int64))[None, :]) % 10
        hd = ((dig + ord("0")) @ pw).astype(np.uint64) & np.uint64(M32 - 1)
        h = ((base + hd * mul + np.uint64(hs)) & np.uint64(M32 - 1)).astype(np.uint32)
        hit = np.nonzero((streams.fmix32(h) & np.uint32(bm)) == bm)[0]
        found += [prefix + b"%0*d" % (digits, lo + int(i)) + suffix for i in hit[:count - len(found)]]
        lo += chunk
    return found


def wrap_family(G, k=6):
    """A collision family of 2^k names whose common home is the last bucket: its chain wraps to bucket 0.  (Every
    member has the hashCode of prefix + "Aa" * k: the prefix is searched with that suffix.)"""
    head = wrap_names(G, 1, prefix=b"w/", digits=8, suffix=PAIRS["ascii"][0] * k)[0]
    return family(k, prefix=head[:-2 * k])


def ordinary_names(rows):
    return [b"svc%d" % int(g) for g in rows]


# ---- the scenario ------------------------------------------------------------------------------------------------

def _ar_frames(names, versions, acceptor=101):
    return [W.batched_accept_reply(nm, int(v), acceptor, 0, 100, 3, [5, 6]) for nm, v in zip(names, versions)]


def _decode(we, frames):
    d = we.decode(frames)
    return [d.f_status.tolist(), d.f_gidx.tolist(), d.f_type.tolist(), d.counts,
            {k: v.tolist() for k, v in d.votes.items()}]


def names_scenario(lib, G, seed, profile=False):
    """Families in one chain each, a chain through the last bucket, ordinary names at normal load; lookups, decodes,
    the coordinator, GPX_S_EXISTS cases, unbinds (tombstones mid-chain, rebuilds), retire / re-create without unbind.
    Returns ([(step, outputs)] to compare, {step: expected lookups or statuses}, whether the tombstone and the
    rebuild steps rebuild the table (the engine's rule), the kernels the engine ran (profile=True))."""
    rng = np.random.default_rng(seed)
    k = 3
    e = Engine(lib, 100, G, kmax=k, window=8, max_batch=1 << 20)
    we = W.WireEngine(e)
    if profile:
        e.profile(2)
    geo = table_geometry(G)
    rows = hri_create(G, k, 100)
    rows["version"] = np.arange(G) % 3
    mem = np.tile(np.array([100, 101, 102], np.int32), (G, 1))
    created = np.arange(G - G // 20, dtype=np.int32)  # the last rows stay without a group
    assert (e.create_groups(created, mem[created], k, rows[created]) == S_OK).all()
    version = np.where(np.arange(G) < created.shape[0], np.arange(G) % 3, 0)

    fams = families()
    fams["wrap-family"] = wrap_family(G)
    fams["wrap-counter"] = wrap_names(G, 12)
    fams["short"] = [b"A", b"\xff", b"\x00", b"z" * 15, b"y" * 16, b"x" * 17, b"v" * 126, b"u" * 127]
    held = {lb: f[-4:] for lb, f in fams.items()}      # same-hash siblings never bound until later
    bound = {lb: f[:-4] for lb, f in fams.items()}
    n_fam = sum(len(f) for f in bound.values())
    perm = rng.permutation(G).astype(np.int32)
    fam_rows = perm[:n_fam]
    n_ord = min(G - n_fam - 64, (G * 7) // 10)        # ordinary names: under one name per bucket on average
    ord_rows = perm[n_fam:n_fam + n_ord]
    free_rows = perm[n_fam + n_ord:]                  # unnamed rows, for the EXISTS and rebinding cases
    out, want = [], {}
    live = {}                                         # row -> name, what every lookup must find

    def bind(step, names, gidx):
        st = we.bind(names, gidx)
        out.append((step, st.tolist()))
        for nm, g, s in zip(names, gidx, st):
            if s == S_OK:
                live[int(g)] = nm
        return st

    def unbind(step, gidx):
        st = we.unbind(gidx)
        out.append((step, st.tolist()))
        for g, s in zip(gidx, st):
            if s == S_OK:
                live.pop(int(g), None)
        return st

    def check_lookups(step, absent):
        names = [live[g] for g in sorted(live)] + list(absent)
        got = we.lookup(names).tolist()
        out.append((step + " lookup", got))
        want[step] = sorted(live) + [-1] * len(absent)

    h1 = n_ord // 2
    bind("ordinary 1", ordinary_names(ord_rows[:h1]), ord_rows[:h1])
    fam_names = [nm for f in bound.values() for nm in f]
    assert (bind("families", fam_names, fam_rows) == S_OK).all()
    bind("ordinary 2", ordinary_names(ord_rows[h1:]), ord_rows[h1:])
    held_names = [nm for f in held.values() for nm in f]
    check_lookups("bound", held_names + [b"", b"A" * 128, b"tenant/0000/svc/", b"svc-absent"])

    # a decode burst addressed to every member (current version, a stale one, the held-back siblings)
    fr = sorted(fam_rows.tolist())
    names_fr = [live[g] for g in fr]
    frames = _ar_frames(names_fr, version[fr]) + _ar_frames(names_fr[::5], version[fr[::5]] + 1) + \
        _ar_frames(held_names, [0] * len(held_names))
    out.append(("decode families", _decode(we, frames)))
    for b in (0, 1, -7):
        out.append(("coordinator %d" % b, W.names_coordinator(we, np.arange(-1, G + 1), b).tolist()))

    # GPX_S_EXISTS: a bound name on a fresh row, a fresh name on a named row; a same-hash sibling on a fresh row is OK
    fx = free_rows[:8]
    bind("exists", [fam_names[0], fam_names[-1], b"svc-new-0", b"svc-new-1", held["len17"][0],
                    held["tail-only"][0]], [fx[0], fx[1], fam_rows[3], ord_rows[0], fx[2], fx[3]])
    want["exists"] = [S_EXISTS, S_EXISTS, S_EXISTS, S_EXISTS, S_OK, S_OK]
    bind("refused lengths", [b"", b"B" * 128], [fx[4], fx[5]])
    want["refused lengths"] = [S_NOGROUP, S_NOGROUP]
    check_lookups("after exists", [b"svc-new-0", b"svc-new-1"])

    # the table's copies of (exists, version): retire named groups without unbinding them, re-create others with a
    # bumped version; frames with the old and the new version, commits and accept replies on those groups
    # (rows that stay bound to the end: the last ordinary names and the family members that are never unbound)
    where = {nm: i for i, nm in enumerate(fam_names)}
    keep = list(ord_rows[-400:]) + [fam_rows[where[nm]] for lb in bound for nm in bound[lb][0::2]]
    keep = np.array([g for g in keep if g < created.shape[0] and int(g) in live], np.int32)
    sel = rng.choice(keep, size=min(600, keep.shape[0]), replace=False).astype(np.int32)
    kill, pause, recreate = sel[0::3], sel[1::3], sel[2::3]

    def copies_round(tag):
        for x, mode in ((kill, RETIRE_KILL), (pause, RETIRE_PAUSE), (recreate, RETIRE_KILL)):
            out.append((tag + " retire", e.retire_groups(x, mode)[1].tolist()))
        r2 = hri_create(recreate.shape[0], k, 100)
        r2["version"] = version[recreate] + 1
        out.append((tag + " re-create", e.create_groups(recreate, mem[recreate], k, r2).tolist()))
        version[recreate] += 1
        q = np.concatenate([kill, pause, recreate])
        nm = [live[int(g)] for g in q]
        frames = _ar_frames(nm, version[q]) + _ar_frames(nm, version[q] - 1)
        out.append((tag + " decode", _decode(we, frames)))
        n = q.shape[0]
        dec = Decisions(q, np.full(n, 1, np.int32), np.zeros(n, np.int32), np.full(n, 100, np.int32),
                        np.zeros(n, np.int32), np.full(n, D_DECISION, np.uint8), np.zeros(0, np.uint8))
        f, fg, nb = we.pack_commits(dec)
        out.append((tag + " pack_commits", [f, fg.tolist(), nb]))
        g2 = np.repeat(q, 2)
        m = g2.shape[0]
        a = we.pack_accept_replies(g2, np.tile([5, 6], n), np.zeros(m, np.int32), np.full(m, 100, np.int32),
                                   np.full(m, 2, np.int32), np.zeros(m, np.uint8))
        out.append((tag + " pack_accept_replies", [a[0], a[1].tolist(), a[2].tolist(), a[3].tolist(), a[4]]))
        out.append((tag + " coordinator", W.names_coordinator(we, q, 3).tolist()))
        # the retired groups come back (same version) for the next round
        for x in (kill, pause):
            r3 = hri_create(x.shape[0], k, 100)
            r3["version"] = version[x]
            out.append((tag + " restore", e.create_groups(x, mem[x], k, r3).tolist()))
        out.append((tag + " decode restored", _decode(we, frames)))

    copies_round("copies")

    # tombstones in the middle of every chain: unbind every other member, then bind the held-back siblings
    drop = np.array([fam_rows[where[nm]] for lb in bound for nm in bound[lb][1::2]], np.int32)
    dropped = [live[int(g)] for g in drop]
    unbind("every other member", drop)
    n_unbind = drop.shape[0]
    rebuilds = [n_unbind > geo["rebuild_after"]]
    assert not rebuilds[0]
    check_lookups("tombstones", dropped)
    sib = [nm for lb in held for nm in held[lb][1:]]
    bind("siblings", sib, free_rows[8:8 + len(sib)])
    check_lookups("siblings", dropped[::3])

    # enough unbinds of ordinary names to cross the rebuild threshold (k_names_reinsert); everything again after it
    need = geo["rebuild_after"] + 1 - n_unbind
    mass = ord_rows[1:][:need]
    assert need + 1 + 400 <= n_ord, "not enough ordinary names to rebuild the table"
    gone = [live[int(g)] for g in mass[::97]]
    unbind("rebuild", mass)
    rebuilds.append(True)
    check_lookups("after rebuild", gone + dropped[1::2])
    bind("rebind after rebuild", dropped[::2], drop[::2])
    check_lookups("rebound", dropped[1::2])
    copies_round("copies after rebuild")
    check_lookups("end", [])
    ran = set(e.profile_read()) if profile else set()
    e.close()
    return out, want, rebuilds, ran
