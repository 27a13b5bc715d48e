"""Host helpers for the eligibility rules of top-N and audience (xmap_rec_filter of include/xmap_hip.h): the packed mask and
the exclusion lists in the layouts the device calls read.  NumPy only."""
import numpy as np


def pack_mask(ids_or_bool, n):
    """The `allow` mask of an id space of n ids as (n + 31) // 32 uint32 words: bit (id & 31) of word (id >> 5) set = id is
    eligible.  ids_or_bool: a bool array [n], or the eligible ids (any order, repeats allowed; an id outside [0, n) is
    ignored).  Bits at or beyond n are zero."""
    n = int(n)
    if n < 0:
        raise ValueError("pack_mask: n = %d" % n)
    a = np.asarray(ids_or_bool)
    if a.dtype == np.bool_:
        if a.shape != (n,):
            raise ValueError("pack_mask: a bool mask of %d ids has shape (%d,), not %s" % (n, n, a.shape))
        on = a
    else:
        if a.size and a.dtype.kind not in "iu":
            raise ValueError("pack_mask: ids must be integers, not %s" % a.dtype)
        ids = a.reshape(-1).astype(np.int64)
        on = np.zeros(n, np.bool_)
        on[ids[(ids >= 0) & (ids < n)]] = True
    padded = np.zeros(((n + 31) // 32) * 32, np.bool_)
    padded[:n] = on
    return np.packbits(padded, bitorder="little").view("<u4").astype(np.uint32)


def exclusion_csr(lists):
    """The exclusion lists of the queries, one sequence of ids per QUERY in query order (None or empty: nothing excluded),
    as (ptr int64 [Q + 1], ids int32): ids[ptr[q] : ptr[q + 1]] are never returned for query q."""
    rows = [np.zeros(0, np.int32) if l is None else np.asarray(list(l), np.int64).reshape(-1) for l in lists]
    ptr = np.zeros(len(rows) + 1, np.int64)
    if rows:
        np.cumsum([len(r) for r in rows], out=ptr[1:])
    flat = np.concatenate(rows) if rows and ptr[-1] else np.zeros(0, np.int64)
    if flat.size and (flat.min() < -2 ** 31 or flat.max() >= 2 ** 31):
        raise ValueError("exclusion_csr: an id does not fit int32")
    return ptr, flat.astype(np.int32)
