/* compiled as C by tests/test_journal_abi.py: the layout of gpx_journal_counts that include/gpx_journal.h promises */
#include <stddef.h>

#include "gpx_journal.h"

_Static_assert(sizeof(gpx_journal_counts) == 32, "gpx_journal_counts is 32 bytes");
_Static_assert(offsetof(gpx_journal_counts, n_bytes) == 16 && offsetof(gpx_journal_counts, bytes_done) == 24,
               "the two byte counts are the third and fourth 8-byte words");
