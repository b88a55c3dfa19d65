/* compiled as C by tests/test_journal_gc_abi.py: the layout of gpx_journal_gc_counts that include/gpx_journal_gc.h promises */
#include <stddef.h>

#include "gpx_journal_gc.h"

_Static_assert(sizeof(gpx_journal_gc_counts) == 64, "gpx_journal_gc_counts is 64 bytes");
_Static_assert(offsetof(gpx_journal_gc_counts, unchanged) == 24 && offsetof(gpx_journal_gc_counts, keep_bytes) == 32 &&
                   offsetof(gpx_journal_gc_counts, bytes_done) == 40 && offsetof(gpx_journal_gc_counts, named_bytes) == 48,
               "eight 4-byte counts, then four 8-byte words");
