/* compiled as C by tests/test_logindex_abi.py: the layout of gpx_logindex_counts that include/gpx_logindex.h promises */
#include <stddef.h>

#include "gpx_logindex.h"

_Static_assert(sizeof(gpx_logindex_counts) == 32, "gpx_logindex_counts is 32 bytes");
_Static_assert(offsetof(gpx_logindex_counts, n_rows) == 0 && offsetof(gpx_logindex_counts, generation) == 8 &&
                   offsetof(gpx_logindex_counts, n_done) == 12 && offsetof(gpx_logindex_counts, n_repeat) == 28,
               "eight 4-byte counts");
