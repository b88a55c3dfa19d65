"""The bucket geometry of an engine, restated from gpx_engine.hip (gpx_engine_create, ar_partition, ar_tiles_call and
tile_shape), and the "hot set" of groups that sits on its edges.  Test infrastructure only: test_geometry_gpu.py and
test_backends_gpu.py assert with gpx_profile_read that the engine launched the kernels this restatement predicts, so
that neither the restatement nor a test can drift onto another path unnoticed."""
import math

import numpy as np

GPX_MIN_SHIFT = 8          # gpx_kernels.hip.h: >= 256 groups per bucket
GPX_MAX_BUCKETS = 4096
V16_MAX_SHIFT = 10         # gpx_ar16.hip.h: one lane per group, at most 1024 lanes
GPX_TL_MAXWG = 1024        # gpx_tiles.hip.h: tiles of one call at most
GPX_SAR_MAX_N = 1024       # gpx_small.hip.h: votes of a call that k_ar_tiny takes
GPX_SAR_MAX_G = 1 << 24
GPX_SMALL_DIRECT_MAX_N = 65536  # gpx_direct.hip.h: ACCEPT / COMMIT / propose batches of one fused launch
RANGE = GPX_MAX_BUCKETS << V16_MAX_SHIFT  # groups of one accept-reply pass beyond 4 M groups (2^22)
CUS = 256                  # compute units of an MI355X
# tile_shape's candidates: (votes, threads) per scatter workgroup and the measured ns of one round of them
TILE_CANDIDATES = [((12288, 1024), 27900), ((8192, 1024), 17300), ((4096, 512), 10000)]
# k_scatter_tiles<NT, R4> instantiations (R4 = T / (NT * 4))
TILE_INSTANCES = {(1024, 1), (1024, 2), (1024, 3), (1024, 4), (512, 2), (512, 4)}


def tl_cnt_words(nbk, nt):
    per = (nbk + 1 + nt - 1) // nt
    return nt * (4 if per <= 4 else 8)


def tl_lds_bytes(nbk, T, NT):
    return tl_cnt_words(nbk, NT) * 4 + T * 8 + 128


def geometry(G, kmax, shift=None):
    """What gpx_engine_create derives from max_groups (and the GPX_BUCKET_SHIFT switch `shift`)."""
    def nbk_for(sh):
        return (G + (1 << sh) - 1) >> sh

    sh = GPX_MIN_SHIFT + 1 if nbk_for(GPX_MIN_SHIFT + 1) >= 256 else GPX_MIN_SHIFT
    while nbk_for(sh) > GPX_MAX_BUCKETS:
        sh += 1
    if shift is not None and GPX_MIN_SHIFT <= shift <= 20 and nbk_for(shift) <= GPX_MAX_BUCKETS:
        sh = shift
    gb = 1 << sh
    threads = min(1024, gb)
    d = dict(G=G, kmax=kmax, shift=sh, gb=gb, nbk=nbk_for(sh), bucket_threads=threads,
             ac16=sh <= V16_MAX_SHIFT and threads == gb)
    if sh <= V16_MAX_SHIFT:
        d.update(shift16=sh, nbk16=d["nbk"], ar_passes=1, lds16_hw=(160 * 1024 - 1024 - gb * 8) // 16)
    else:
        d.update(shift16=V16_MAX_SHIFT, nbk16=GPX_MAX_BUCKETS, ar_passes=(G + RANGE - 1) // RANGE,
                 lds16_hw=(160 * 1024 - 1024 - (1 << V16_MAX_SHIFT) * 8) // 16)
    return d


def ar_passes(geo, n):
    """ar_partition: the passes over ascending group ranges of a (partitioned) call of n votes."""
    NB = (geo["G"] + (1 << geo["shift16"]) - 1) >> geo["shift16"]
    m = n / NB
    pc = int((m + 5.0 * math.sqrt(m)) / geo["lds16_hw"]) + 1
    want = min(NB, max(geo["ar_passes"], pc))
    bpp = (NB + want - 1) // want
    return (NB + bpp - 1) // bpp


def tile_shape(nbk, n, force_T=0, force_NT=0, cus=CUS):
    """tile_shape, then ar_tiles_call's own correction: (T, NT) of a tiled call, or None where it refuses."""
    if force_T:
        T, NT = force_T, force_NT or (512 if force_T <= 8192 else 1024)
    else:
        best, cost = (4096, 512), None
        for (T, NT), round_ns in TILE_CANDIDATES:
            if tl_lds_bytes(nbk, T, NT) > 158 * 1024:
                continue
            nwg = (n + T - 1) // T
            if nwg > GPX_TL_MAXWG:
                continue
            c = (nwg + cus - 1) // cus * round_ns + nwg * 5
            if cost is None or c < cost:
                best, cost = (T, NT), c
        T, NT = best
    if nbk + 1 > NT * 8:  # every bucket's counter and the one behind the last: 4,096 buckets need 1024 threads
        NT = 1024
    if T not in (4096, 8192, 12288, 16384) or NT not in (512, 1024) or T % (NT * 4):
        return None
    if (NT, T // (NT * 4)) not in TILE_INSTANCES or tl_lds_bytes(nbk, T, NT) > 158 * 1024:
        return None
    if (n + T - 1) // T > GPX_TL_MAXWG:
        return None
    return T, NT


def ar_route(geo, n, tiles=True, sar_max_n=GPX_SAR_MAX_N, force_T=0, force_NT=0):
    """The front end of a shuffled accept-reply call of n votes (aligned columns, no runs promise):
    'tiny', ('tiles', T, NT) or ('partition', passes)."""
    if n <= sar_max_n and geo["G"] <= GPX_SAR_MAX_G:
        return ("tiny",)
    passes = ar_passes(geo, n)
    if tiles and passes == 1 and geo["nbk16"] <= GPX_MAX_BUCKETS and 8 <= geo["shift16"] <= 10:
        ts = tile_shape(geo["nbk16"], n, force_T, force_NT)
        if ts is not None:
            return ("tiles",) + ts
    return ("partition", passes)


def ar_kernels(route):
    """Kernels an accept-reply call launches on `route` (ar_route's answer)."""
    if route[0] == "tiny":
        return {"k_ar_tiny"}
    if route[0] == "tiles":
        return {"k_scatter_tiles", "k_emit_dec16"}
    return {"k_hist", "k_scatter_ar16", "k_bucket_ar16", "k_emit_dec16"}


def ac_kernels(geo, n, op):
    """Kernels an unpromised ACCEPT (op 'accept') or COMMIT ('commit') batch of n records launches (both back ends:
    the device picks the one that works)."""
    ks = {"k_ac_small"} if n <= GPX_SMALL_DIRECT_MAX_N else {"k_order_check", "k_ac_direct", "k_emit_runs_direct"}
    if geo["ac16"]:
        ks |= {"k_scatter_ac16", "k_bucket_%s16" % op, "k_emit_runs16"}
    else:
        ks |= {"k_hist", "k_scatter_ac", "k_bucket_%s" % op, "k_emit_runs"}
    return ks


def hot_set(G, geo, rng, extra=2000):
    """A few thousand groups on the table's edges; returns (sorted gidx, {placement: gidx that stand for it})."""
    gb, nbk = geo["gb"], geo["nbk"]
    gb16 = 1 << geo["shift16"]
    place = {}
    place["first bucket"] = np.arange(0, min(G, 64))
    last0 = (nbk - 1) * gb
    place["last bucket"] = np.unique(np.concatenate([np.arange(last0, min(G, last0 + 64)), np.arange(max(last0, G - 64), G)]))
    bs = np.unique(np.concatenate([np.arange(1, min(nbk, 9)), np.arange(max(1, nbk - 8), nbk),
                                   rng.integers(1, max(nbk, 2), 16)]))
    bs = bs[(bs >= 1) & (bs < nbk)]
    place["bucket boundaries"] = np.unique(np.concatenate([bs * gb - 1, bs * gb]))
    # the accept-reply passes' own buckets (1024 groups beyond 4 M groups)
    b16 = np.unique(np.concatenate([np.arange(1, 5), rng.integers(1, max((G + gb16 - 1) // gb16, 2), 16)]))
    b16 = b16[b16 * gb16 < G]
    place["accept-reply bucket boundaries"] = np.unique(np.concatenate([b16 * gb16 - 1, b16 * gb16]))
    if G > RANGE:
        place["range boundary"] = np.arange(RANGE - 4, min(G, RANGE + 4))
    if gb > 1024:
        # lanes l, l + 1024, l + 2048, ... of one bucket: one thread applies them all
        b = (nbk - 1) // 2
        ls = np.array([0, 1, 511, 1023])
        place["shared threads"] = np.unique(np.concatenate([b * gb + ls + j * 1024 for j in range(gb // 1024)]))
        place["shared threads (last bucket)"] = np.unique(np.concatenate(
            [last0 + ls + j * 1024 for j in range(gb // 1024)]))
    place = {k: v[(v >= 0) & (v < G)].astype(np.int32) for k, v in place.items()}
    hot = np.unique(np.concatenate(list(place.values()) + [rng.integers(0, G, extra)])).astype(np.int32)
    return hot, place


# The fuzz cells of test_backends_gpu.py: the switches that pick a back end (set before the HIP engine is created) and
# the fuzz's shape.  `refused`: the operations that the cell's stream gets refused with GPX_S_WINDOW at least once
# (proposals only fill a window of 4 or 8 in the cells marked so: the fuzz keeps the proposal frontier within its slot
# span, and most groups lose the coordinator role to the stream's other ballots first).  test_geometry_model.py runs
# every cell oracle against oracle on the CPU and checks `refused`; the fuzz draws the same stream whichever engine
# answers, so the GPU cells' window legs are not vacuous either.
FUZZ_SPAN = 40
CELLS = {
    "partition-k3-w4": dict(refused=("propose", "accept", "commit"), env=dict(GPX_SAR_MAX_N=0, GPX_AR_TILES=0), kmax=3, window=4, G=600, seed=61, steps=120, batch=800),
    "partition-k5-w8": dict(refused=("propose", "accept", "commit"), env=dict(GPX_SAR_MAX_N=0, GPX_AR_TILES=0), kmax=5, window=8, G=600, seed=62, steps=120, batch=800),
    "partition-k8-w32": dict(refused=("accept", "commit"), env=dict(GPX_SAR_MAX_N=0, GPX_AR_TILES=0), kmax=8, window=32, G=600, seed=63, steps=120, batch=800),
    "partition-k16-w8": dict(refused=("propose", "accept", "commit"), env=dict(GPX_SAR_MAX_N=0, GPX_AR_TILES=0), kmax=16, window=8, G=600, seed=64, steps=120, batch=800),
    "tiles-k3-w8": dict(refused=("accept", "commit"), env=dict(GPX_SAR_MAX_N=0), kmax=3, window=8, G=700, seed=71, steps=80, batch=3000, min_batch=1025),
    "tiles-k8-w4": dict(refused=("propose", "accept", "commit"), env=dict(GPX_SAR_MAX_N=0), kmax=8, window=4, G=700, seed=72, steps=80, batch=3000, min_batch=1025),
    "runs-k5-w32": dict(refused=("accept", "commit"), env=dict(GPX_SAR_MAX_N=0, GPX_TRY_RUNS=1), kmax=5, window=32, G=500, seed=81, steps=80, batch=1500),
    "runs-k3-w4": dict(refused=("propose", "accept", "commit"), env=dict(GPX_SAR_MAX_N=0, GPX_TRY_RUNS=1), kmax=3, window=4, G=400, seed=82, steps=80, batch=1500),
    "big-accept-commit-k3-w8": dict(refused=("accept", "commit"), env={}, kmax=3, window=8, G=1024, seed=91, steps=12, batch=90_000, min_batch=66_000,
                                    max_batch=1 << 17),
    "wide-s11-w8": dict(refused=("propose", "accept", "commit"), env=dict(GPX_BUCKET_SHIFT=11), shift=11, kmax=3, window=8, G=3000, seed=103, steps=150, batch=1200),
    "wide-s12-w4": dict(refused=("propose", "accept", "commit"), env=dict(GPX_BUCKET_SHIFT=12), shift=12, kmax=3, window=4, G=9000, seed=102, steps=150, batch=1200),
}


def cell_gmap(c):
    """The fuzzed rows of a wide cell: a hot set with lanes l, l + 1024, ... of one bucket (None: rows 0 .. G-1)."""
    if "shift" not in c:
        return None
    return hot_set(c["G"], geometry(c["G"], c["kmax"], c["shift"]), np.random.default_rng(c["seed"]), extra=300)[0]


def run_cell(lib_a, lib_b, c, kmax=None, seed=None, ordered=False, profile=False, steps=None, counted=None):
    """One fuzz cell: engine a against engine b.  Returns (statuses seen per operation, kernels engine a launched).
    steps: another number of fuzz steps than the cell's own.  counted: a wrapper class for engine a that counts its
    calls (tests/lifetime_common.py: Counted); the answer is then (statuses, the wrapper, {kernel: launches})."""
    from tests.parity_common import make_pair, create_mixed_groups, fuzz
    kmax = c["kmax"] if kmax is None else kmax
    seed = c["seed"] if seed is None else seed
    rng = np.random.default_rng(seed)
    nodes = [100, 101, 102, 103, 104, 105, 106, 107] if kmax <= 8 else list(range(100, 120))
    gmap = cell_gmap(c)
    G = c["G"]
    H = G if gmap is None else gmap.shape[0]
    ea, eb = make_pair(lib_a, lib_b, 100, G, kmax, c["window"], max_batch=c.get("max_batch", 1 << 16))
    create_mixed_groups(ea, eb, H, kmax, nodes, rng, gmap=gmap)
    profile = profile and "profile_enable" in ea.lib.fn   # (the oracle has no kernels to name)
    if profile:
        ea.profile(2)
    ef = ea if counted is None else counted(ea)
    seen = fuzz(ef, eb, H, nodes, rng, steps=c["steps"] if steps is None else steps, batch=c["batch"],
                min_batch=c.get("min_batch", 1), gmap=gmap, ordered=ordered, span=c.get("span", FUZZ_SPAN))
    prof = ea.profile_read() if profile else {}
    ea.close()
    eb.close()
    if counted is not None:
        return seen, ef, {k: v[0] for k, v in prof.items()}
    return seen, set(prof)
