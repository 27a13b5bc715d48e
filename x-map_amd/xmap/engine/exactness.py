"""When are the plain fp64 sums of cosine mode exact?

Cosine mode sums, per item, r and r^2 over its raters and, per item pair, r_i r_j over their co-raters.  Adjusted cosine
and the canonical value sum exactly and round once; plain fp64 adds give the same bits whenever
every partial sum is exact, whatever the order.  That holds when every rating is a multiple of 2^-e and
U M^2 2^2e <= 2^53 (M = max |r|, U = users, the most terms a sum can have): then every term is an integer multiple of
2^-2e and no partial sum needs more than 53 bits.  The engine keeps the fast kernels (LDS atomics, plain adds) for such
ratings and takes the double-double route (XMAP_COSINE_EXACT) otherwise.  XMAP_EXACT_COSINE=1 forces that route.
The coarse C ABI applies the same rule when ratings are uploaded (csrc/api.hip: plain_sums_exact).
"""
import os

import numpy as np

MAX_FRAC_BITS = 26      # 2e <= 53 at U = M = 1


def fraction_bits(rating):
    """least e with every rating * 2^e an integer (None: above MAX_FRAC_BITS, or a non-finite rating)"""
    r = np.abs(np.asarray(rating, np.float64).ravel())
    if not np.all(np.isfinite(r)):
        return None
    for e in range(MAX_FRAC_BITS + 1):
        x = np.ldexp(r, e)
        if np.array_equal(x, np.floor(x)):
            return e
    return None


def plain_sums_exact(rating, n_users, env=True):
    """True when cosine mode's plain fp64 sums over these ratings are exact in any order (see the module docstring).
    env: honour XMAP_EXACT_COSINE=1 (-> False)."""
    if env and os.environ.get("XMAP_EXACT_COSINE") == "1":
        return False
    r = np.asarray(rating, np.float64).ravel()
    if r.size == 0:
        return True
    e = fraction_bits(r)
    if e is None:
        return False
    M = float(np.abs(r).max())
    if M == 0.0:
        return True
    Mi = int(np.ldexp(M, e))                 # an integer: M is a multiple of 2^-e
    return int(n_users) * Mi * Mi <= 2 ** 53
