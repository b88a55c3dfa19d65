"""A stand-in engine for checking the fuzz driver itself: it forwards every call to a real engine and folds the
call's name and input columns into a hash, so that two versions of a driver can be shown to send the same stream."""
import hashlib

import numpy as np


class RecordingEngine:
    def __init__(self, inner):
        self._e = inner
        self.h = hashlib.sha256()

    def __getattr__(self, name):
        return getattr(self._e, name)

    def _wrap(name):
        def call(self, *args):
            self.h.update(name.encode())
            for a in args:
                if a is None:
                    self.h.update(b"-")
                elif isinstance(a, np.ndarray):
                    self.h.update(str(a.dtype).encode() + np.ascontiguousarray(a).tobytes())
                else:
                    self.h.update(repr(a).encode())
            return getattr(self._e, name)(*args)
        return call

    propose = _wrap("propose")
    accept = _wrap("accept")
    accept_reply = _wrap("accept_reply")
    commit = _wrap("commit")
    prepare = _wrap("prepare")

    def hexdigest(self):
        return self.h.hexdigest()
