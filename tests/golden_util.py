"""Helpers shared by the parity tests: load tests/golden/*.npz (vectors captured from the
reference by oracle/ref_harness/make_golden.py) into index-space inputs."""
import os

import numpy as np

from xmap.engine import ids as xids

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["kat7", "tiny", "mixed", "multilabel", "small", "medium", "fractional"]
# cases with non-integer ratings: the reference's left-to-right fp64 sums (item sums, cosine dot) round there, the
# canonical value is the exact sum rounded once -- sums to FRACTIONAL_RTOL, every discrete output still exact
FRACTIONAL = {"fractional"}
FRACTIONAL_RTOL = 1e-13
METHODS = ["cosine", "adjust_cosine"]
CAP = 50


class Golden(object):
    def __init__(self, name):
        self.name = name
        self.g = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
        self.iids = [str(s) for s in self.g["iids"]]
        self.uids = [str(s) for s in self.g["uids"]]
        self.I = len(self.iids)
        self.attrs = xids.item_attrs(self.iids)
        self.ptr = self.g["train_ptr"]
        self.item = self.g["train_item"]
        self.rating = self.g["train_rating"].astype(np.float32)
        self.time = self.g["train_time"]

    def __getitem__(self, k):
        return self.g[k]

    def has(self, k):
        return k in self.g.files

    def ks(self, method):
        out = set()
        for f in self.g.files:
            p = f.split(".")
            if p[0] == method and len(p) > 2 and p[1].startswith("k"):
                out.add(int(p[1][1:]))
        return sorted(out)

    def gen_tags(self, method, k):
        pre = "%s.k%d." % (method, k)
        tags = set()
        for f in self.g.files:
            if f.startswith(pre):
                t = f[len(pre):].split(".")[0]
                if t == "priv" or t.startswith("np"):
                    tags.add(t)
        return sorted(tags)

    def oracle_train(self):
        from oracle import xmap_oracle as xo
        return xo.Train(self.ptr, self.item, self.rating, self.time, self.I, *self.attrs)


def csr_to_pairs(row_ptr, col):
    rows = np.repeat(np.arange(len(row_ptr) - 1, dtype=np.int64), np.diff(row_ptr))
    return rows, col.astype(np.int64)


def census(So, Xo, m, ae):
    """How much work stages B and C do on one input, from the oracle's results alone (stage A `So`, extension `Xo`,
    replacement map `m`, AlterEgo rows `ae`): a comparison with the oracle proves something about the path kernels, the
    selection and the aggregation only where these are not zero."""
    n_cand = np.diff(Xo.xs_ptr)
    return dict(nb=int(((Xo.bb == 0) & (np.diff(So.row_ptr) > 0)).sum()),      # non-bridge items with a similarity row
                paths=int(Xo.n_paths), n_out=int(len(Xo.xs_end)),
                starts=int((n_cand > 0).sum()),                                # starts with a candidate
                max_cand=int(n_cand.max()) if len(n_cand) else 0,              # the longest candidate list
                neg=int((Xo.xs_val < 0).sum()),                                # candidates with a negative X-Sim
                mapped=int((np.asarray(m) >= 0).sum()),                        # items with a replacement
                mapped_rows=int(len(ae["user"]) - ae["n_target_rows"]))        # AlterEgo rows made of replaced items


def check_census(got, need, what=""):
    """`need`: lower bounds on entries of census(); a missed one fails with the whole census in the message"""
    unknown = sorted(set(need) - set(got))
    assert not unknown, "census has no quantity %s" % unknown
    missed = {n: (got[n], lo) for n, lo in need.items() if got[n] < lo}
    assert not missed, "%s: the input does too little work for this test, (measured, required) = %s; census %s" % (what, missed, got)


def with_gaps(r, seed):
    """r (a synth.Ratings) in stretched index spaces, as a host that does not compact its ids uploads it: 0 to 3 unrated
    item indices before every item plus runs of more than 1500 at index 0, across the source / target boundary (each domain
    owns part of that run) and at the end; 0 to 2 users without ratings before every user plus runs of more than 70 at the
    start, 1100 in the middle and 300 at the end.  The order of items and users is kept, so every result of the stretched
    input is the compact input's re-indexed.  -> (Ratings, new index of every item, new index of every user)"""
    from xmap.engine import synth
    rng = np.random.default_rng(seed)
    I, Is, U = r.n_items, r.n_src_items, r.n_users
    assert 0 < Is < I and U > 2
    gap = rng.integers(0, 4, I)
    gap[0] += 1500 + rng.integers(0, 64)
    mid = 1500 + int(rng.integers(0, 64))
    gap[Is] += mid
    item_map = np.cumsum(gap + 1) - 1
    n_src = int(item_map[Is]) - int(rng.integers(1, mid))          # the boundary lies inside the middle run
    n_items = int(item_map[-1]) + 1 + 1500 + int(rng.integers(0, 64))
    ugap = rng.integers(0, 3, U)
    ugap[0] += 70 + rng.integers(0, 8)
    ugap[U // 2] += 1100 + rng.integers(0, 64)
    user_map = np.cumsum(ugap + 1) - 1
    n_users = int(user_map[-1]) + 1 + 300 + int(rng.integers(0, 16))
    length = np.zeros(n_users, np.int64)
    length[user_map] = np.diff(r.user_ptr)
    ptr = np.zeros(n_users + 1, np.int64)
    np.cumsum(length, out=ptr[1:])
    g = synth.Ratings(ptr, item_map[r.item].astype(np.int32), r.rating, r.time, n_items, n_src, np.arange(n_src),
                      np.arange(n_items - n_src))
    assert item_map[Is - 1] < n_src <= item_map[Is] and g.nnz == r.nnz
    return g, item_map, user_map


# what the entries of a result are, for reindexed(): per item / per user arrays (with the value of an index that has no
# counterpart) and arrays whose values are item or user indices (-1 = none stays)
_PER_ITEM = dict(info=0, n_cand=0, top_end=-1, top_val=0, bb=0, cls=0, kcnt=0, kcol=-1, kval=0, n_top=0, choice=-1, map=-1)
_PER_USER = dict(uavg=0)
_ITEM_VALUED = ("rows", "cols", "item", "top_end", "kcol", "choice", "map")
_USER_VALUED = ("user",)


def reindexed(res, item_map, user_map, n_items, n_users):
    """the results of a compact input (a dict as test_gpu_coarse_oracle's driver returns them; `lists` = (start, end,
    value)) as its stretched form (with_gaps) must return them: indices mapped, per-item and per-user arrays scattered,
    an unrated item without info, class, candidates or replacement, a user without ratings with average 0.0"""
    def values(name, a):
        a = np.asarray(a)
        m = item_map if name in _ITEM_VALUED else user_map if name in _USER_VALUED else None
        if m is None:
            return a
        return np.where(a >= 0, m[np.maximum(a, 0)], -1).astype(a.dtype)
    out = {}
    for name, a in res.items():
        if name == "lists":
            out[name] = (item_map[a[0]].astype(a[0].dtype), item_map[a[1]].astype(a[1].dtype), a[2])
            continue
        a = values(name, a)
        if name in _PER_ITEM or name in _PER_USER:
            m, n, fill = (item_map, n_items, _PER_ITEM[name]) if name in _PER_ITEM else (user_map, n_users, _PER_USER[name])
            full = np.full((n,) + a.shape[1:], fill, a.dtype)
            full[m] = a[:len(m)]
            a = full
        out[name] = a
    return out


def rows_to_csr(rows):
    """(uid, iid, rating, ts)* -> (uids, iids, user_ptr, item, rating) with users in order of first appearance and items
    in lexicographic id order (the index space of the engine and of the oracle)."""
    import numpy as np
    uids, useen = [], {}
    for r in rows:
        if r[0] not in useen:
            useen[r[0]] = len(uids)
            uids.append(r[0])
    iids = sorted({r[1] for r in rows})
    iidx = {s: k for k, s in enumerate(iids)}
    per = [[] for _ in uids]
    for r in rows:
        per[useen[r[0]]].append((iidx[r[1]], float(r[2])))
    ptr = np.zeros(len(uids) + 1, np.int64)
    item, rating = [], []
    for k, prof in enumerate(per):
        ptr[k + 1] = ptr[k] + len(prof)
        item += [p[0] for p in prof]
        rating += [p[1] for p in prof]
    return uids, iids, ptr, np.array(item, np.int32), np.array(rating, np.float64)     # fp64: AlterEgo ratings are np.float64 means
