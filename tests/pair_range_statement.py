"""The designed model of the tests at the launch limit of the pair kernels (tests/test_cpu_pair_ranges.py,
tests/test_gpu_pair_ranges.py), and its expected results as a closed form.  NumPy only.

Item 0 is `h`, the one item anybody holds; it has no list and the average 0.  Items 1 .. Q have the neighbour list [h] with the
similarity +0.5 or -0.5 and an average that is a multiple of 8, each multiple once; item Q + 1 has an empty list.  Users
0 .. U - 1 hold one row of h, rated 1 + pi(u) / 2^17 with a fixed permutation pi of 0 .. U - 1; the users U, U + 1, U + 2 hold h
128, 129 and 300 times at distinct times, rated m - d and m + d in turns (and m once where the count is odd), all multiples
of 1 / 16: their mean is m = 2.5, 3 and 3.5.  keep = 1 and the decay table is all ones.

The evidence of a pair (u, q) is the rows of h that u holds: e0 = sim[q] * (rating - 0), e1 = 0.5.  With one row, sum(e0) /
sum(e1) = (+-0.5 r) / 0.5 = +-r; with n rows the left-to-right sums are exact (multiples of 1 / 32 below 2^10) and their ratio
is +-m.  So every score is  avg[q] + sign[q] * R[u]  with R[u] the rating of a short user and the mean of a long one -- a
multiple of 2^-17 below 2^13, exact in fp64, the same plain and decayed, distinct within a user (the averages are 8 apart,
R < 4) and within an item (R is distinct).  test_cpu_pair_ranges.py checks each of these sentences."""
import numpy as np

Q = 1000                    # items with a list
U = 70000                   # users with one row
LONG = (128, 129, 300)      # rows of the users U, U + 1, U + 2
LONG_MEAN = (2.5, 3.0, 3.5)
N_W = 304                   # entries of the decay table: max_now = 301 needs 301
THREADS_LIMIT_PAIRS = 67108861      # the smallest pair count whose single grid ((pairs + 3) / 4 blocks of 256) has 2^32 threads
N_PAIRS_A = THREADS_LIMIT_PAIRS + 4099 + 2
EXPLAIN_LIMIT_PAIRS = 4194304       # with 16 entries per pair: 2^32 threads of xmap_explain_sources
N_PAIRS_D = EXPLAIN_LIMIT_PAIRS + 5


def permutation(n_users):
    """pi: a fixed permutation of 0 .. n_users - 1 (a multiplier coprime to n_users)"""
    a = 48271
    while np.gcd(a, n_users) != 1:
        a += 2
    return (np.arange(n_users, dtype=np.int64) * a + 12345) % n_users


def long_rows(count, mean):
    """(ratings, times) of a long user: mean -+ d in turns, d = (1 + k % 8) / 16; distinct times in an order that is not the
    rows' order"""
    d = (1 + (np.arange(count // 2) % 8)) / 16.0
    r = np.empty(count)
    r[0:2 * (count // 2):2] = mean - d
    r[1:2 * (count // 2):2] = mean + d
    if count % 2:
        r[-1] = mean
    t = (np.arange(count, dtype=np.int64) * 7) % count if np.gcd(7, count) == 1 else (np.arange(count, dtype=np.int64) * 11) % count
    return r, 1000 + 60 * t


def model(n_users=U, n_lists=Q):
    """dict of the arrays of xmap_predict_rows / xmap_topn_rows / xmap_audience_rows (ptr, item, rating, time, cnt, col, sim, avg),
    the sizes, and the closed form's tables: sign [I] (0 for an item without a list) and R [n_users + 3]"""
    I, n_all = n_lists + 2, n_users + len(LONG)
    counts = np.concatenate([np.ones(n_users, np.int64), np.asarray(LONG, np.int64)])
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rating = np.empty(int(ptr[-1]))
    time = np.empty(int(ptr[-1]), np.int64)
    rating[:n_users] = 1.0 + permutation(n_users) / 131072.0
    time[:n_users] = 500 + np.arange(n_users) % 3
    for k, (c, m) in enumerate(zip(LONG, LONG_MEAN)):
        rating[ptr[n_users + k]:ptr[n_users + k + 1]], time[ptr[n_users + k]:ptr[n_users + k + 1]] = long_rows(c, m)
    item = np.zeros(int(ptr[-1]), np.int32)
    q = np.arange(1, n_lists + 1)
    cnt, col, sim, avg = np.zeros(I, np.int32), np.full((I, 1), -1, np.int32), np.zeros((I, 1)), np.zeros(I)
    cnt[q], col[q, 0] = 1, 0
    sim[q, 0] = np.where((q * 7 + q // 3) % 5 < 2, -0.5, 0.5)
    # the multiples of 8 from -8 * (n_lists // 2) up, each once, in an order that is not the items'
    step = 387 if np.gcd(387, n_lists) == 1 else 1
    avg[q] = 8.0 * (((q * step) % n_lists) - n_lists // 2)
    sim[q[avg[q] == 0.0], 0] = 0.5          # the item whose bounded predictions differ from user to user: 1 .. 4
    avg[I - 1] = 4.0            # the item with the empty list
    sign = np.zeros(I)
    sign[q] = 2.0 * sim[q, 0]
    R = np.concatenate([rating[:n_users], LONG_MEAN])
    return dict(arrays=[ptr, item, rating, time, cnt, col, sim, avg], n_users=n_all, n_short=n_users, n_items=I, n_lists=n_lists, keep=1,
                sign=sign, R=R, wtab=np.ones(N_W))


def loop_score(M, u, q):
    """the score of (u, q) as the kernel and the Python statement sum it: left to right, in fp64.  (plain, decayed, entries)"""
    ptr, _, rating, time, _, _, sim, avg = M["arrays"]
    a, b = int(ptr[u]), int(ptr[u + 1])
    s = float(sim[q, 0])
    p0 = p1 = 0.0
    for p in range(a, b):
        p0 += s * (float(rating[p]) - 0.0)
        p1 += abs(s)
    d0 = d1 = 0.0
    for p in sorted(range(a, b), key=lambda p: time[p]):
        d0 += (s * (float(rating[p]) - 0.0)) * 1.0
        d1 += abs(s) * 1.0
    return float(avg[q]) + p0 / p1, float(avg[q]) + d0 / d1, b - a


def closed_scores(M, users=None):
    """[n_users + 3][I] (or [len(users)][I]) of avg[q] + sign[q] * R[u]; the columns of the items without a list mean nothing"""
    R = M["R"] if users is None else M["R"][np.asarray(users)]
    return M["arrays"][7][None, :] + M["sign"][None, :] * R[:, None]


def bound_rating(x):
    """max(0, min(int(x + 0.5), 5)) of the reference's bound_rating, vectorised"""
    x = np.asarray(x, np.float64) + 0.5
    return np.where(x >= 5.0, 5.0, np.where(x < 1.0, 0.0, np.trunc(x)))


def closed_topn(M, users, n):
    """per query user the n best items with a list: (items [len(users)][n], scores) by (-score, item); every user has evidence for
    every such item and holds none of them"""
    S = closed_scores(M, users)[:, 1:M["n_lists"] + 1]
    order = np.argsort(- S, axis=1, kind="stable")[:, :n]
    return (order + 1).astype(np.int32), np.take_along_axis(S, order, axis=1)


def closed_audience(M, items, n):
    """per query item the n best users: (users [len(items)][n], scores) by (-score, user)"""
    S = closed_scores(M)[:, np.asarray(items)].T
    order = np.argsort(- S, axis=1, kind="stable")[:, :n]
    return order.astype(np.int32), np.take_along_axis(S, order, axis=1)


# ------------------------------------------------------------------- the raw-profile model of the explanation's sources
def raw_profile_model(n_users, seed):
    """the hand-made map of test_gpu_explain._tiny_case (items 0..3 target, 4..7 source; the sources 5 and 6 merge onto target 1,
    7 goes to 3, 4 is not mapped) under n_users raw profiles of 1 .. 12 entries, every ninth of 65 .. 90 (items repeat; longer
    than one wave's chunk of 64): the AlterEgo profile of a user is its pass-through rows in raw order, then one mapped row per
    target in the order the targets first appear.  (ptr, item, cnt_t, raw_ptr, raw_item, flags, map)"""
    rng = np.random.default_rng(seed)
    flags = np.asarray([2, 2, 2, 2, 1, 1, 1, 1], np.uint8)
    m = np.asarray([-1, -1, -1, -1, -1, 1, 1, 3], np.int32)
    raw, prof, cnt_t = [], [], []
    for u in range(n_users):
        n = int(rng.integers(1, 13)) if u % 9 else int(rng.integers(65, 91))
        r = rng.integers(0, 8, n).astype(np.int32)
        if u % 50 == 0:
            r = r[m[r] < 0] if (m[r] < 0).any() else np.asarray([4], np.int32)        # a user without a mapped row
        rows = [int(x) for x in r if flags[x] & 2]
        cnt_t.append(len(rows))
        seen = []
        for x in r:
            if m[x] >= 0 and int(m[x]) not in seen:
                seen.append(int(m[x]))
        raw.append(r)
        prof.append(rows + seen)
    ptr = np.concatenate([[0], np.cumsum([len(p) for p in prof])]).astype(np.int64)
    raw_ptr = np.concatenate([[0], np.cumsum([len(r) for r in raw])]).astype(np.int64)
    return (ptr, np.asarray([x for p in prof for x in p], np.int32), np.asarray(cnt_t, np.int32), raw_ptr,
            np.concatenate(raw).astype(np.int32), flags, m)
