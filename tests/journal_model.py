"""The journal batches of include/gpx_journal.h, restated over numpy and bytes, and two readers of the bytes.

`pack` is the header: the selection by status and GPX_R_TOLOG, both frame forms, the frame test and n_bad, the entry
bytes `<be32 len><frame>` in record order, the index rows, both caps and base_offset.  `logbatch` is FileLogger::
logBatch's loop (gigapaxos_amd/host/gpx_host.cpp) on its own.  `read_entry` is getJournaledMessage (SQLPaxosLogger.java:
3077-3096) - seek(offset), readInt() == length, read length bytes - written without looking at `pack`; `walk` is what
recovery does with a file whose tail may be torn."""
import struct
from collections import namedtuple

import numpy as np

S_OK, S_NOGROUP, S_WINDOW = 0, 1, 3
R_TOLOG, R_STORED = 1, 2
COUNT_ONLY = 1
MAX_LEN = 2 ** 31 - 1 - 4
ROW_COLS = ("rec", "gidx", "slot", "bnum", "bcoord", "off", "len")

Packed = namedtuple("Packed", "bytes rows counts frames")   # rows: {column: array}; counts: dict; frames: done frames


def frame_range(frame_off, frame_len, n_frames, frames_bytes, f):
    """(start, length) of frame f, or None where it cannot be used"""
    if not 0 <= f < n_frames:
        return None
    s = int(frame_off[f])
    ln = int(frame_len[f]) if frame_len is not None else int(frame_off[f + 1]) - s
    if s < 0 or ln < 0 or ln > MAX_LEN or s + ln > frames_bytes:
        return None
    return s, ln


def pack(frames, frame_off, gidx, slot, bnum, bcoord, r_flags, status, frame_len=None, rec_frame=None, base_offset=0,
         flags=0, cap_bytes=None, cap_entries=None, n_frames=None, frames_bytes=None):
    """gpx_journal_pack on host data.  cap_bytes / cap_entries None: no cut."""
    frames = bytes(frames)
    frames_bytes = len(frames) if frames_bytes is None else frames_bytes
    if n_frames is None:
        n_frames = len(frame_off) - (1 if frame_len is None else 0)
    n = len(status)
    ents, bad, pos = [], 0, 0
    for i in range(n):
        if int(status[i]) != S_OK or not int(r_flags[i]) & R_TOLOG:
            continue
        r = frame_range(frame_off, frame_len, n_frames, frames_bytes, int(rec_frame[i]) if rec_frame is not None else i)
        if r is None:
            bad += 1
            continue
        ents.append((i, r[0], r[1], pos))
        pos += 4 + r[1]
    done = []
    if not flags & COUNT_ONLY:
        for e, (i, s, ln, p) in enumerate(ents):
            if (cap_entries is not None and e >= cap_entries) or (cap_bytes is not None and p + 4 + ln > cap_bytes):
                break
            done.append((i, s, ln, p))
    out = b"".join(struct.pack(">i", ln) + frames[s:s + ln] for _, s, ln, _ in done)
    idx = np.array([i for i, _, _, _ in done], np.int64)
    rows = {"rec": idx.astype(np.int32), "gidx": np.asarray(gidx, np.int32)[idx], "slot": np.asarray(slot, np.int32)[idx],
            "bnum": np.asarray(bnum, np.int32)[idx], "bcoord": np.asarray(bcoord, np.int32)[idx],
            "off": np.array([base_offset + p for _, _, _, p in done], np.int64),
            "len": np.array([ln for _, _, ln, _ in done], np.int32)} if not flags & COUNT_ONLY else None
    counts = dict(n_entries=len(ents), n_done=len(done), n_bad=bad, reserved=0, n_bytes=pos, bytes_done=len(out))
    return Packed(out, rows, counts, [frames[s:s + ln] for _, s, ln, _ in done])


def counts_of(c):
    """a JournalCounts structure as the model's dict"""
    return dict(n_entries=c.n_entries, n_done=c.n_done, n_bad=c.n_bad, reserved=c.reserved, n_bytes=c.n_bytes,
                bytes_done=c.bytes_done)


def logbatch(frames):
    """FileLogger::logBatch: length-prefixed records, one after the other"""
    out = bytearray()
    for f in frames:
        n = len(f)
        for sft in (24, 16, 8, 0):
            out.append((n >> sft) & 0xFF)
        out += f
    return bytes(out)


class JournalFile:
    """the log file as getJournaledMessage sees it: a RandomAccessFile whose first byte is at file offset `base`"""

    def __init__(self, data, base=0):
        self.data, self.base, self.pos = bytes(data), base, 0

    def seek(self, offset):
        self.pos = offset - self.base

    def read_int(self):
        if self.pos < 0 or self.pos + 4 > len(self.data):
            raise EOFError
        v = int.from_bytes(self.data[self.pos:self.pos + 4], "big", signed=True)
        self.pos += 4
        return v

    def read_fully(self, n):
        if self.pos + n > len(self.data):
            raise EOFError
        b = self.data[self.pos:self.pos + n]
        self.pos += n
        return b


def read_entry(data, offset, length, base=0):
    """getJournaledMessage: raf.seek(offset); assert raf.readInt() == length; raf.readFully(new byte[length])"""
    raf = JournalFile(data, base)
    raf.seek(offset)
    got = raf.read_int()
    assert got == length, (offset, got, length)
    return raf.read_fully(length)


def walk(data, base=0):
    """the whole entries of a file that may end torn: ([offset], [length], good_bytes)"""
    raf = JournalFile(data, base)
    offs, lens = [], []
    while True:
        at = raf.pos
        try:
            ln = raf.read_int()
            if ln < 0:
                raise EOFError
            raf.read_fully(ln)
        except EOFError:
            return offs, lens, at
        offs.append(base + at)
        lens.append(ln)
