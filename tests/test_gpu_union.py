"""The union of the AlterEgo rows of several two-domain problems as one set of user-major profiles, on the device
(csrc/stage_c_union.hip: xmap_union_count / xmap_union_fill; Engine.union_profiles; session.union_alterego; xmap_ctx_union),
and the recommender tail over it.

The reference statement is brute force, written here: per union user concatenate the parts in the order given -- within a part
the local user's pass-through rows, then its mapped rows --, map the items, drop the rows that map to -1 and remove duplicates
with a set of (item, rating, time) tuples (Python floats: -0.0 == 0.0 and they hash alike).  Compared byte for byte."""
import ctypes as C
import datetime

import numpy as np
import pytest

from golden_util import CAP
from test_gpu_coarse_abi import Ctx, _p
from test_gpu_tail import (_check_item_avg, _check_rec_sim, _few_times, _oracle_rec, device_tuples, dicts_from_arrays, generate,
                           make_pairs, neighbors, predict, rec_sim, select, statement as predict_statement, wtab)
from test_gpu_topn import check_output, expected, recommend, score_users

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHORT, MED = 32, 2048           # the class boundaries of csrc/stage_c_union.hip (UN_SHORT, UN_MED), in rows of a union user


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.zeros(1, device="cuda")


def test_the_class_boundaries_are_the_kernels():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "x-map_amd", "csrc", "stage_c_union.hip")).read()
    assert int(re.search(r"constexpr int UN_SHORT = (\d+);", src).group(1)) == SHORT
    assert int(re.search(r"constexpr int UN_MED = (\d+);", src).group(1)) == MED


# ------------------------------------------------------------------------------------------------ parts and the statement
class Part(object):
    """one domain's stage-C output as NumPy arrays + its maps.  users: per local user (pass-through rows, mapped rows), each a
    list of (local item, rating, time)"""

    def __init__(self, users, user_map, item_map):
        pt = [row for t, _ in users for row in t]
        mp = [row for _, m in users for row in m]
        rows = pt + mp
        self.n_users, self.n_items = len(users), len(item_map)
        self.n_rows, self.n_target_rows = len(rows), len(pt)
        self.user = np.asarray([u for u, (t, _) in enumerate(users) for _ in t] + [u for u, (_, m) in enumerate(users) for _ in m], np.int32)
        self.item = np.asarray([r[0] for r in rows], np.int32)
        self.rating = np.asarray([r[1] for r in rows], np.float64)
        self.time = np.asarray([r[2] for r in rows], np.int64)
        self.off_t = np.concatenate([[0], np.cumsum([len(t) for t, _ in users])]).astype(np.int64)
        self.off_m = np.concatenate([[0], np.cumsum([len(m) for _, m in users])]).astype(np.int64)
        self.user_map = np.asarray(user_map, np.int32)
        self.item_map = np.asarray(item_map, np.int32)

    @classmethod
    def of_arrays(cls, rows, off_t, off_m, n_target_rows, user_map, item_map):
        """from downloaded stage-C rows (dict of user / item / rating / time)"""
        p = object.__new__(cls)
        p.n_users, p.n_items, p.n_rows, p.n_target_rows = len(off_t) - 1, len(item_map), len(rows["item"]), int(n_target_rows)
        p.user, p.item, p.rating, p.time = rows["user"], rows["item"], rows["rating"], rows["time"]
        p.off_t, p.off_m = np.asarray(off_t, np.int64), np.asarray(off_m, np.int64)
        p.user_map, p.item_map = np.asarray(user_map, np.int32), np.asarray(item_map, np.int32)
        return p


def union_statement(parts, n_users, n_items, distinct):
    """(prof_ptr, item, rating, time, counts) of the contract, by brute force"""
    per = [[] for _ in range(n_users)]
    dropped = 0
    for p in parts:
        item, rating, time = p.item.tolist(), p.rating.tolist(), p.time.tolist()
        imap = p.item_map.tolist()
        for u in range(p.n_users):
            g = int(p.user_map[u])
            spans = ((int(p.off_t[u]), int(p.off_t[u + 1])), (p.n_target_rows + int(p.off_m[u]), p.n_target_rows + int(p.off_m[u + 1])))
            for a, b in spans:
                for e in range(a, b):
                    it = imap[item[e]]
                    if it < 0:
                        dropped += 1
                    else:
                        per[g].append((it, rating[e], time[e]))
    dups, out = 0, []
    ptr = np.zeros(n_users + 1, np.int64)
    for g, rows in enumerate(per):
        seen = set()
        for row in rows:
            if distinct:
                if row in seen:
                    dups += 1
                    continue
                seen.add(row)
            out.append(row)
        ptr[g + 1] = len(out)
    return (ptr, np.asarray([r[0] for r in out], np.int32), np.asarray([r[1] for r in out], np.float64),
            np.asarray([r[2] for r in out], np.int64), (len(out), dups, dropped, int((np.diff(ptr) > 0).sum())))


SENT = -77


def union_rc(parts, n_users, n_items, flags, n_target_rows=None):
    """xmap_union_count (+ xmap_union_fill) on device copies of the parts; the outputs start as a sentinel.  Returns
    (rc, ptr, item, rating, time, counts)"""
    import torch
    from xmap.engine import hipabi as abi
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    keep, desc = [], (abi.UnionPart * len(parts))()
    for d, p in enumerate(parts):
        t = [to(x) for x in (p.user, p.item, p.rating, p.time, p.off_t, p.off_m, p.user_map, p.item_map)]
        keep.append(t)
        nt = p.n_target_rows if n_target_rows is None else n_target_rows[d]
        desc[d] = abi.UnionPart(p.n_users, p.n_items, p.n_rows, nt, *[x.data_ptr() for x in t])
    st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    ptr = torch.full((n_users + 1,), SENT, dtype=torch.int64, device=DEV)
    h = (C.c_int64 * 4)(SENT, SENT, SENT, SENT)
    rc = abi.lib.xmap_union_count(st, len(parts), desc, n_users, n_items, flags, abi.vp(ptr), h)
    torch.cuda.synchronize()
    if rc:
        return rc, ptr.cpu().numpy(), None, None, None, tuple(h)
    n = int(h[0])
    item = torch.full((n + 3,), SENT, dtype=torch.int32, device=DEV)
    rating = torch.full((n + 3,), float(SENT), dtype=torch.float64, device=DEV)
    time = torch.full((n + 3,), SENT, dtype=torch.int64, device=DEV)
    abi.check(abi.lib.xmap_union_fill(st, len(parts), desc, n_users, n_items, flags, abi.vp(ptr), n, abi.vp(item), abi.vp(rating), abi.vp(time)))
    torch.cuda.synchronize()
    item, rating, time = item.cpu().numpy(), rating.cpu().numpy(), time.cpu().numpy()
    assert (item[n:] == SENT).all() and (rating[n:] == SENT).all() and (time[n:] == SENT).all()      # nothing behind the counted size
    return 0, ptr.cpu().numpy(), item[:n], rating[:n], time[:n], tuple(h)


def check_union(got, want):
    rc, ptr, item, rating, time, counts = got
    assert rc == 0
    assert counts == want[4]
    assert np.array_equal(ptr, want[0]) and np.array_equal(item, want[1]) and np.array_equal(time, want[3])
    assert np.array_equal(rating.view(np.uint64), want[2].view(np.uint64))


# ------------------------------------------------------------------------------------------------------ 1. hand-made parts
N_ITEMS, N_DROP = 60, 5         # union items; local items that map to -1 (the last N_DROP of every part)
LENGTHS = (1, 2, SHORT - 1, SHORT, SHORT + 1, 2 * SHORT, 2 * SHORT + 1, 300, MED - 1, MED, MED + 1, 5000)


def _hand_parts(D):
    """D parts over one union space, described per union user in union items and turned into every part's own index space.
    Returns (parts, n_users, {name: union user})"""
    rng = np.random.default_rng(100 + D)
    perm = [rng.permutation(N_ITEMS) for _ in range(D)]             # local item -> union item, + N_DROP items that map to -1
    inv = [np.argsort(p) for p in perm]
    spec, names = [], {}                                            # per union user: {part: (pass-through rows, mapped rows)}

    def user(name, by_part):
        names[name] = len(spec)
        spec.append(by_part)
    same = [(3, 4.0, 10), (7, 2.5, 11)]
    # pass-through rows identical across ALL parts (all but the first removed), mapped rows of its own in every part
    user("all", {d: (list(same), [(20 + d, 1.0 + d, 5)]) for d in range(D)})
    user("one", {0: ([(1, 1.0, 1)], [(2, 2.0, 2), ("drop", 3.0, 3)])})
    # first occurrence in part 0, the next in the LAST part only (part 2 of 3: part 1 holds the user without that row)
    user("far", {0: ([(9, 3.0, 7)], [(8, 1.0, 1)]), **({1: ([], [(8, 1.5, 1)])} if D > 2 else {}), D - 1: ([(5, 5.0, 5)], [(9, 3.0, 7)])})
    user("none", {})                                                # a union user with no rows, named by no part
    user("empty-local", {0: ([], []), D - 1: ([], [])})             # named by local users that have no rows
    # inside ONE part: an exact duplicate; equal (item, time), other rating; equal (item, rating), other time; 0.0 and -0.0
    user("inside", {D - 1: ([(4, 2.0, 3), (4, 2.0, 3), (4, 2.5, 3), (4, 2.0, 4)], [(6, 0.0, 9), (6, -0.0, 9), (6, 0.0, 8), (4, 2.0, 3)])})
    user("negzero-first", {0: ([(6, -0.0, 9)], []), D - 1: ([(6, 0.0, 9)], [(6, -0.0, 9)])})
    user("all-dropped", {0: ([("drop", 1.0, 1)], [("drop", 2.0, 2)])})
    for L in LENGTHS:                                               # both sides of every class boundary, and beyond the LDS class
        span = int(np.ceil(np.sqrt(L))) + 1
        cut = np.sort(rng.integers(0, L + 1, 2 * D - 1))
        sizes = np.diff(np.concatenate([[0], cut, [L]]))
        by_part = {}
        for d in range(D):
            segs = []
            for k in (0, 1):
                rows = []
                for _ in range(int(sizes[2 * d + k])):
                    x = int(rng.integers(0, min(N_ITEMS, span)))
                    rows.append(("drop" if rng.random() < 0.05 else x, [1.0, 2.5][int(rng.integers(0, 2))], int(rng.integers(0, span // 2 + 1))))
                segs.append(rows)
            by_part[d] = tuple(segs)
        user("len%d" % L, by_part)
    n_users = len(spec)
    parts = []
    for d in range(D):
        gs = [g for g in range(n_users) if d in spec[g]]
        order = rng.permutation(len(gs))
        users, user_map = [], []
        for k in order:
            t, m = spec[gs[k]][d]
            loc = lambda rows: [(N_ITEMS + int(rng.integers(0, N_DROP)) if x == "drop" else int(inv[d][x]), ra, tm) for x, ra, tm in rows]
            users.append((loc(t), loc(m)))
            user_map.append(gs[k])
        parts.append(Part(users, user_map, np.concatenate([perm[d], np.full(N_DROP, -1)])))
    return parts, n_users, names


_HAND = {}


def _hand(D, distinct):
    if D not in _HAND:
        parts, n_users, names = _hand_parts(D)
        _HAND[D] = (parts, n_users, names, {f: union_statement(parts, n_users, N_ITEMS, bool(f)) for f in (0, 1)})
    parts, n_users, names, want = _HAND[D]
    return parts, n_users, names, want[distinct]


@pytest.mark.parametrize("D", [2, 3])
def test_the_hand_made_case_holds_what_it_should(D):
    """the statement's own output shows every kind of user the case is there for (no device involved)"""
    parts, n_users, names, want = _hand(D, 1)
    plain = _hand(D, 0)[3]
    rows = lambda w, g: list(zip(w[1][w[0][g]:w[0][g + 1]].tolist(), w[2][w[0][g]:w[0][g + 1]].tolist(), w[3][w[0][g]:w[0][g + 1]].tolist()))
    g = names["all"]
    assert len(rows(plain, g)) == 3 * D and len(rows(want, g)) == 2 + D
    assert rows(want, names["far"]).count((9, 3.0, 7)) == 1 and rows(plain, names["far"]).count((9, 3.0, 7)) == 2
    assert not rows(want, names["none"]) and not rows(want, names["empty-local"]) and not rows(plain, names["all-dropped"])
    inside = rows(want, names["inside"])
    assert inside == [(4, 2.0, 3), (4, 2.5, 3), (4, 2.0, 4), (6, 0.0, 9), (6, 0.0, 8)]
    bits = lambda w, g: w[2][w[0][g]:w[0][g + 1]].view(np.uint64).tolist()
    assert bits(want, names["inside"])[3] == 0                                          # 0.0 came first: its bits stay
    assert bits(want, names["negzero-first"]) == [1 << 63]                              # -0.0 came first: its bits stay
    for L in LENGTHS:
        g = names["len%d" % L]
        n_in = sum(int(p.off_t[u + 1] - p.off_t[u] + p.off_m[u + 1] - p.off_m[u]) for p in parts for u in range(p.n_users) if p.user_map[u] == g)
        assert n_in == L
        if L > 2:
            assert len(rows(want, g)) < len(rows(plain, g)) <= L
    g = names["len5000"]
    assert 0.3 < len(rows(want, g)) / 5000.0 < 0.7                                      # about half of them duplicates
    assert want[4][1] > 0 and want[4][2] > 0 and 0 < want[4][3] < n_users
    assert any((p.item_map == -1).any() for p in parts) and any(p.n_users < n_users for p in parts)


@pytest.mark.parametrize("D,distinct", [(2, 1), (2, 0), (3, 1), (3, 0)])
def test_hand_made_parts_equal_the_statement(D, distinct):
    parts, n_users, _, want = _hand(D, distinct)
    got = union_rc(parts, n_users, N_ITEMS, distinct)
    check_union(got, want)
    again = union_rc(parts, n_users, N_ITEMS, distinct)                                 # a pure function of the inputs
    assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(got[1:5], again[1:5])) and got[5] == again[5]


def test_one_part_and_empty_inputs():
    parts, n_users, _, _ = _hand(2, 1)
    for distinct in (0, 1):
        check_union(union_rc(parts[:1], n_users, N_ITEMS, distinct), union_statement(parts[:1], n_users, N_ITEMS, bool(distinct)))
    none = Part([], [], [])
    check_union(union_rc([none], 0, 0, 1), union_statement([none], 0, 0, True))
    check_union(union_rc([none, none], 5, 3, 1), union_statement([none, none], 5, 3, True))
    rowless = Part([([], []), ([], [])], [3, 0], [0, -1])
    check_union(union_rc([rowless], 4, 1, 1), union_statement([rowless], 4, 1, True))


# ----------------------------------------------------------------------------------- 2. more users than a grid dimension
def test_more_users_than_a_grid_dimension():
    rng = np.random.default_rng(5)
    n_users, n_items = 70000, 40
    parts = []
    for d in range(2):
        U = 60000 + 5000 * d
        user_map = rng.permutation(n_users)[:U]
        n_t, n_m = rng.integers(0, 2, U), rng.integers(0, 2, U)
        n = int(n_t.sum() + n_m.sum())
        rows = dict(user=np.concatenate([np.repeat(np.arange(U), n_t), np.repeat(np.arange(U), n_m)]).astype(np.int32),
                    item=rng.integers(0, 8, n).astype(np.int32), rating=rng.integers(1, 3, n).astype(np.float64),
                    time=rng.integers(0, 2, n).astype(np.int64))
        item_map = np.concatenate([rng.permutation(n_items)[:7], [-1]])
        parts.append(Part.of_arrays(rows, np.concatenate([[0], np.cumsum(n_t)]), np.concatenate([[0], np.cumsum(n_m)]), int(n_t.sum()),
                                    user_map, item_map))
    for distinct in (1, 0):
        want = union_statement(parts, n_users, n_items, bool(distinct))
        assert np.diff(want[0]).max() <= 4 and (np.diff(want[0]) == 0).any() and want[4][2] > 0
        check_union(union_rc(parts, n_users, n_items, distinct), want)
    assert want[4][1] == 0 and union_statement(parts, n_users, n_items, True)[4][1] > 0


# ------------------------------------------------------------------------------------------- 3. every kind of bad input
def _small_parts():
    rng = np.random.default_rng(9)
    parts = []
    for d in range(2):
        users = [([(int(rng.integers(0, 6)), float(rng.integers(1, 4)), int(rng.integers(0, 3))) for _ in range(int(rng.integers(0, 4)))],
                  [(int(rng.integers(0, 6)), float(rng.integers(1, 4)), int(rng.integers(0, 3))) for _ in range(int(rng.integers(1, 4)))])
                 for _ in range(9)]
        parts.append(Part(users, rng.permutation(12)[:9], np.concatenate([rng.permutation(10)[:5], [-1]])))
    return parts


def _edited(parts, d, **fields):
    import copy
    out = [copy.copy(p) for p in parts]
    for k, v in fields.items():
        setattr(out[d], k, v)
    return out


def test_every_kind_of_bad_input_is_refused_before_anything_is_indexed():
    from xmap.engine import hipabi as abi
    parts = _small_parts()
    n_users, n_items = 12, 10
    want = union_statement(parts, n_users, n_items, True)
    check_union(union_rc(parts, n_users, n_items, 1), want)
    p1 = parts[1]

    def edit(a, k, v):
        a = a.copy()
        a[k] = v
        return a
    swapped = p1.off_m.copy()
    k = int(np.nonzero(np.diff(p1.off_m) > 0)[0][0])
    swapped[k], swapped[k + 1] = swapped[k + 1], swapped[k]
    assert (np.diff(swapped) < 0).any()
    bad = {
        "user_map entry too large": (_edited(parts, 1, user_map=edit(p1.user_map, 4, n_users)), None, "user_map entry outside"),
        "user_map entry negative": (_edited(parts, 0, user_map=edit(parts[0].user_map, 0, -1)), None, "user_map entry outside"),
        "item_map entry too large": (_edited(parts, 1, item_map=edit(p1.item_map, 2, n_items)), None, "item_map entry outside"),
        "item_map entry below -1": (_edited(parts, 1, item_map=edit(p1.item_map, 0, -2)), None, "item_map entry outside"),
        "user_map not injective": (_edited(parts, 1, user_map=edit(p1.user_map, 3, int(p1.user_map[7]))), None, "twice"),
        "offsets not monotone": (_edited(parts, 1, off_m=swapped), None, "off_m"),
        "off_t does not start at 0": (_edited(parts, 0, off_t=parts[0].off_t + 1), None, "off_t"),
        "off_t disagrees with n_target_rows": (parts, [parts[0].n_target_rows, p1.n_target_rows + 1], "off_"),
        "off_m disagrees with n_rows": (_edited(parts, 1, off_m=edit(p1.off_m, -1, int(p1.off_m[-1]) - 1)), None, "off_m"),
        "row item too large": (_edited(parts, 1, item=edit(p1.item, p1.n_rows - 1, p1.n_items)), None, "row item outside"),
        "row item negative": (_edited(parts, 0, item=edit(parts[0].item, 0, -1)), None, "row item outside"),
    }
    for name, (ps, nt, text) in bad.items():
        rc, ptr, _, _, _, counts = union_rc(ps, n_users, n_items, 1, n_target_rows=nt)
        assert rc == abi.ERR_ARG, name
        assert text in abi.lib.xmap_last_error().decode(), (name, abi.lib.xmap_last_error())
        assert (ptr == SENT).all() and counts == (SENT,) * 4, name                      # no output written
        if "part 1" in abi.lib.xmap_last_error().decode():
            assert ps[1] is not parts[1] or nt is not None
    check_union(union_rc(parts, n_users, n_items, 1), want)                             # a valid call afterwards
    check_union(union_rc(parts, n_users, n_items, 0), union_statement(parts, n_users, n_items, False))


# ------------------------------------------------------------------------------------------------------ 4. trained shape
def _trained_domains(kind, D):
    """D source domains with shared users (equal indices) and one target catalogue, identified by the target items' numbers:
    `two`: synth.make_two_domain per source -- the catalogues overlap, a user's target ratings differ between the domains;
    `multi`: synth.make_multi_domain -- one set of target entries shared by all (pass-through rows equal across the domains);
    overlap 0.15: with many more shared users every item of so small a catalogue is a bridge item and stage B finds no path"""
    from xmap.engine import synth
    if kind == "multi":
        return [_few_times(r) for r in synth.make_multi_domain(21, 400, 150, 120, D, overlap=0.15)]
    return [_few_times(synth.make_two_domain(31 + d, 400, 150, 120, overlap=0.45)) for d in range(D)]


def _train_parts(doms, k=5):
    """stage A -> B -> C per domain through the engine; [(G, user_map, item_map, None)*], the downloaded rows as Parts, sizes"""
    from xmap.engine import device
    numbers = np.unique(np.concatenate([r.tgt_numbers for r in doms]))
    U = doms[0].n_users
    parts, host = [], []
    for r in doms:
        eng = device.Engine(device.DeviceRatings(r.user_ptr, r.item, r.rating, r.time, r.n_items, r.item_attrs(), DEV))
        E = eng.extend(eng.item_sim("cosine", CAP), k)
        G = eng.alterego(eng.select(E, True)[2])
        assert G.n_rows > G.n_target_rows > 0
        user_map = np.arange(U, dtype=np.int32)
        item_map = np.full(r.n_items, -1, np.int32)
        item_map[r.n_src_items:] = np.searchsorted(numbers, r.tgt_numbers)
        parts.append((G, user_map, item_map, None))
        rows = dict(user=G.user.cpu().numpy(), item=G.item.cpu().numpy(), rating=G.rating.cpu().numpy(), time=G.time.cpu().numpy())
        host.append(Part.of_arrays(rows, G.off_t.cpu().numpy(), G.off_m.cpu().numpy(), G.n_target_rows, user_map, item_map))
    return parts, host, U, len(numbers)


@pytest.mark.parametrize("kind,D", [("two", 2), ("two", 3), ("multi", 3)])
def test_trained_domains_through_the_engine(kind, D):
    import torch
    from test_gpu_recsim import _oracle_pairs, _pairs
    from oracle import xmap_oracle as xo
    from xmap.engine import device
    parts, host, U, I = _train_parts(_trained_domains(kind, D))
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    for distinct in (False, True):
        want = union_statement(host, U, I, distinct)
        P = device.Engine.union_profiles(parts, U, I, distinct=distinct)
        assert P.counts == want[4] and P.n_users == U and P.n_items == I and P.nnz == want[4][0]
        n = P.nnz
        ptr, pit, pra, ptm = P.user_ptr.cpu().numpy(), P.user_item.cpu().numpy()[:n], P.user_rating64.cpu().numpy()[:n], P.user_time.cpu().numpy()[:n]
        assert np.array_equal(ptr, want[0]) and np.array_equal(pit, want[1]) and np.array_equal(ptm, want[3])
        assert np.array_equal(pra.view(np.uint64), want[2].view(np.uint64))
    assert want[4][2] == 0 and (want[4][1] > 0 or kind != "multi")             # shared target entries are duplicates
    assert (P.flags.cpu().numpy() == 2).all()                                  # every union item a target item
    # RecommenderSim and the selection over the union, bit for bit with the oracle over the same profiles
    e2 = device.Engine(P)
    S = e2.rec_sim(CAP)
    O = xo.rec_sim(ptr, pit, pra, I, CAP)
    a, b, sim, ls, nij = _pairs(S, I)
    orow, ocol, osim, ols, onij = _oracle_pairs(O, I)
    assert len(a) > 0 and np.array_equal(a, orow) and np.array_equal(b, ocol) and np.array_equal(nij, onij)
    assert np.array_equal(sim.view(np.uint64), osim.view(np.uint64)) and np.array_equal(ls.view(np.uint64), ols.view(np.uint64))
    assert np.array_equal(S.norm.cpu().numpy(), O.norm)
    avg = S.info[:I, 0].contiguous()
    T = dict(item=pit, rating=pra, avg=avg.cpu().numpy())
    _check_item_avg(T, I)
    for keep in (1, 10):
        nb = e2.rec_select(S, keep)
        ocnt, ocol2, osim2, ols2 = xo.rec_select(O, keep)
        cnt, col, sim2, ls2 = [x.cpu().numpy() for x in nb]
        assert np.array_equal(cnt, ocnt) and np.array_equal(col, ocol2)
        assert np.array_equal(sim2.view(np.uint64), osim2.view(np.uint64)) and np.array_equal(ls2.view(np.uint64), ols2.view(np.uint64))
    xo.rec_free(O)
    # prediction and top-N: the Python statements over the downloaded union profiles
    rows = dict(user=np.repeat(np.arange(U, dtype=np.int32), np.diff(ptr)), item=pit, rating=pra, time=ptm)
    rng = np.random.default_rng(3)
    alpha = 1.5
    tu = rng.integers(0, U, 600).astype(np.int32)
    ti = rng.choice(np.unique(pit), 600).astype(np.int32)
    tu[5::23] = -1
    real = rng.integers(1, 6, 600).astype(np.float64).tolist()
    w = to(wtab(alpha, 66))
    plain, decay, status, max_now = e2.predict(P, nb, to(tu), to(ti), avg, w)
    ratings, sims, info = dicts_from_arrays(rows, I, T["avg"], S.norm.cpu().numpy(), (cnt, col, sim2))
    wanted = predict_statement(alpha, tu.tolist(), ti.tolist(), real, ratings, sims, info)
    assert None not in wanted and max_now <= 66 and sum(1 for t in wanted if t != ()) > 100
    assert device_tuples(ti.tolist(), real, plain.cpu().numpy(), decay.cpu().numpy(), status.cpu().numpy()) == wanted
    m = e2.mae(status, to(np.asarray(real)), plain, decay).tolist()
    got = [t for t in wanted if t != ()]
    assert m[0] == len(got) and m[1] == sum(abs(t[1] - t[2]) for t in got) and m[2] == sum(abs(t[1] - t[3]) for t in got)
    queries = np.concatenate([rng.integers(0, U, 150), [-1, U + 3]]).astype(np.int32)
    scored = score_users(alpha, queries, ptr, pit, pra, ptm, cnt, col, sim2, T["avg"], 10)
    for n_top, rank_by, held in ((10, 0, False), (10, 1, False), (3, 1, True)):
        out = e2.topn(P, nb, to(queries), avg, w, n_top, rank_by, held)
        check_output([x.cpu().numpy() for x in out[:4]] + [out[4]], expected(scored, queries, n_top, rank_by, held, 66), n_top)
    assert any(len(l) for l in expected(scored, queries, 10, 0, False, 66)[0])


# ------------------------------------------------------------------------------------------------------ 5. session route
def test_session_route_equals_the_dict_fed_pipeline():
    """two source domains against one target through the drop-in API; the comparison pipeline is the multi-domain example's:
    alterEgo.union(profile).distinct() -> recommender_calculate_sim_pipeline -> non-private selection -> item_based_recommendation"""
    from pyspark import SparkContext, SparkConf
    from pyspark.sql import SQLContext
    from test_gpu_topn import _tool
    from test_gpu_topn_eval import discounts, relevant_sets, statement as eval_statement
    from xmap.core.baselinerSim import BaselinerSim
    from xmap.core.extender import ExtendSim
    from xmap.core.generator import Generator
    from xmap.core.recommenderPrediction import RecommenderPrediction
    from xmap.core.recommenderPrivacy import RecommenderPrivacy
    from xmap.core.recommenderSim import RecommenderSim
    from xmap.engine import session, synth
    from xmap.engine.localrdd import LocalRDD
    from xmap.utils import assist
    doms = synth.make_multi_domain(17, 600, 200, 150, 2, overlap=0.4)
    t0 = datetime.datetime(2013, 3, 1)
    sc = SparkContext(conf=SparkConf())
    tool = BaselinerSim("cosine", CAP)
    handles = []
    for d, r in enumerate(doms):
        # times that do not grow with the row position, with ties -- and the same object for a target rating in both domains
        recs = [(u, [(i, ra, t0 + datetime.timedelta(days=(t * 7919) % 6)) for i, ra, t in prof]) for u, prof in r.train_records()]
        if d == 1:
            recs = recs[::-1]                                   # the parts' user orders differ: the user maps are no identity
        trainRDD = sc.parallelize(recs, 8).cache()
        sim = assist.baseliner_calculate_sim_pipeline(sc, tool, trainRDD)
        ext = assist.extender_pipeline(sc, SQLContext(sc), tool, ExtendSim(5), sim)
        handles.append(assist.generator_pipeline(Generator(1, 0.6, "cosine", 0.1), trainRDD, ext, True))
    h1, h2 = handles
    union = session.union_alterego([h1, h2])
    host_rows = h1.union(h2).distinct()
    assert union.collect() == host_rows.collect()
    assert session.union_alterego([h1, h2], distinct=False).collect() == h1.union(h2).collect()
    n_all, n_distinct = h1.count() + h2.count(), host_rows.count()
    assert union.counts == (n_distinct, n_all - n_distinct, 0, len({row[0] for row in host_rows.collect()})) and n_distinct < n_all
    # ---- recommend: the dict-fed pipeline with its own neighbour lists, which both routes use
    rsim = RecommenderSim("cosine_item", CAP)
    _, _, ubd, ibd, uinfo, iinfo, alterEgo_sim = assist.recommender_calculate_sim_pipeline(sc, rsim, host_rows)
    kept = assist.recommender_privacy_pipeline(RecommenderPrivacy(10, 0.6, 0.1), alterEgo_sim, False).collectAsMap()
    rng = np.random.default_rng(17)
    iids = sorted({row[1] for row in host_rows.collect()})
    uids = doms[0].user_ids()
    test = []
    for q in range(300):
        uid = uids[int(rng.integers(0, len(uids)))] if q % 29 else "A%013d" % (10 ** 9 + q)
        pairs = [(iids[int(x)], float(rng.integers(1, 6)), t0) for x in rng.choice(len(iids), int(rng.integers(1, 5)), replace=False)]
        if q % 13 == 0:
            pairs.append((doms[0].item_ids()[0], 3.0, t0))      # a source item: no list
        test.append((uid, pairs))
    testRDD = LocalRDD(test)
    for alpha in (0.03, 1.5):
        ptool = RecommenderPrediction(alpha, "cosine_item")
        want = ptool.item_based_recommendation(testRDD, ibd, sc.broadcast(kept), iinfo)
        out = session.recommend(union, testRDD, CAP, 10, alpha, neighbors=kept)
        assert out.collect() == want.collect()
        assert any(p == () for _, ps in want.collect() for p in ps) and sum(1 for _, ps in want.collect() for p in ps if p != ()) > 100
        w_plain, w_decay = [float(x) for x in ptool.calculate_mae(want).split(";")]
        assert ptool.calculate_mae(out) == ptool.calculate_mae(want)
        assert out.mae[0] == sum(1 for _, ps in want.collect() for p in ps if p != ())
        assert out.mae[1] / out.mae[0] == w_plain and out.mae[2] / out.mae[0] == w_decay
    # ---- recommend_topn: the statement on id strings, from the dictionaries of the result
    alpha = 1.5
    ptool = _tool(alpha)
    item_based = rsim.build_sthbased_profile(host_rows, "item").collectAsMap()
    query = [uids[int(x)] for x in rng.integers(0, len(uids), 80)] + ["A%013d" % (10 ** 9 + 1)]
    mine = {uid: {} for uid in query}
    for iid, lst in item_based.items():
        for who, ra, when in lst:
            if who in mine:
                mine[who].setdefault(iid, []).append((ra, when))

    def topn_statement(sim_pairs, item_info, n, decay, keep_held):
        res = []
        for uid in query:
            cand = []
            for iid in sorted(sim_pairs):
                if not keep_held and iid in mine[uid]:
                    continue
                ev = [(s * (ra - item_info[nid][0]), abs(s), when) for nid, s in sim_pairs[iid] for ra, when in mine[uid].get(nid, ())]
                if ev:
                    base = item_info[iid][0]
                    cand.append((iid, base + sum(e[0] for e in ev) / sum(e[1] for e in ev), float(base + ptool._decayed_ratio(ev))))
            cand.sort(key=lambda c: (- c[2 if decay else 1], c[0]))
            res.append((uid, cand[:n]))
        return res
    for n, decay, keep_held in ((10, False, False), (5, True, True)):
        top = session.recommend_topn(union, query, CAP, 10, alpha, n, decay=decay, keep_held=keep_held)
        assert top.collect() == topn_statement(top.sim_pairs, top.item_info, n, decay, keep_held)
        assert top.stats[0] > 0 and top.stats[1] == 0 and top.collect()[-1] == (query[-1], [])
    assert any(len(l) == 5 for _, l in top.collect())
    # ---- evaluate_topn: the lists of recommend_topn for the users with a relevant pair, scored by the definition
    idt = union.state.idt
    seen, held_out = set(), []
    for uid, pairs in test:
        keep_pairs = [p for p in pairs if (uid, p[0]) not in seen and not seen.add((uid, p[0]))]
        held_out.append((uid, keep_pairs))
    tu = np.asarray([idt.uidx.get(uid, -1) for uid, ps in held_out for _ in ps], np.int32)
    ti = np.asarray([idt.iidx.get(p[0], -1) for _, ps in held_out for p in ps], np.int32)
    tr = np.asarray([p[1] for _, ps in held_out for p in ps], np.float64)
    U, I = len(idt.uids), len(idt.iids)
    n_rel, rel, counts = relevant_sets(tu, ti, tr, 4.0, U, I)
    users = np.nonzero(n_rel)[0]
    ev = session.evaluate_topn(union, LocalRDD(held_out), CAP, 10, alpha, 10, cutoffs=(1, 5, 10), rel_min=4.0)
    lists = session.recommend_topn(union, [idt.uids[u] for u in users], CAP, 10, alpha, 10).collect()
    cnt = np.asarray([len(l) for _, l in lists], np.int32)
    item = np.full((len(lists), 10), -1, np.int32)
    for q, (_, l) in enumerate(lists):
        item[q, :len(l)] = [idt.iidx[c[0]] for c in l]
    w_mask, _, w_agg, w_cover = eval_statement(tu, ti, tr, 4.0, U, I, n_rel, rel, users, cnt, item, (1, 5, 10), discounts(10))
    assert ev.stats[:4] == (len(users),) + tuple(counts) and len(users) > 50 and counts[1] > 0
    assert ev.masks == {idt.uids[u]: int(m) for u, m in zip(users.tolist(), w_mask.tolist())}
    for k, c in enumerate((1, 5, 10)):
        m, n_ev = ev.at[c], w_agg[k, 0]
        assert m["users"] == n_ev == len(users) and m["coverage"] == w_cover[k]
        assert [m["hit_rate"], m["precision"], m["recall"], m["ndcg"], m["map"], m["mrr"]] == [w_agg[k, 1] / n_ev] + [x / n_ev for x in w_agg[k, 3:]]
    assert w_mask.any()
    # ---- fold-in needs one replacement map
    late = [("L1", [(doms[0].item_ids()[0], 4.0, t0)])]
    with pytest.raises(TypeError, match="one replacement map"):
        session.recommend_topn_profiles(union, late, CAP, 10, alpha, 5)
    with pytest.raises(TypeError, match="one replacement map"):
        session.recommend_profiles(union, late, LocalRDD([("L1", [(iids[0], 4.0, t0)])]), CAP, 10, alpha)
    with pytest.raises(TypeError):
        session.union_alterego([h1, LocalRDD(h2.collect())])


# ----------------------------------------------------------------------------------------------- 6. coarse ABI, NumPy only
def _union(dst, srcs, user_maps, item_maps, n_users, n_items, flags):
    """xmap_ctx_union: (rc, counts)"""
    hs = (C.c_void_p * len(srcs))(*[s.h.value for s in srcs])
    um = (C.c_void_p * len(srcs))(*[a.ctypes.data for a in user_maps])
    im = (C.c_void_p * len(srcs))(*[a.ctypes.data for a in item_maps])
    counts = np.full(4, -7, np.int64)
    rc = dst.lib.xmap_ctx_union(dst.h, len(srcs), hs, um, im, n_users, n_items, flags, _p(counts, C.c_int64))
    return rc, tuple(counts.tolist())


def _tail_answers(ctx, I, U, n_rows, tu, ti, real, queries, held):
    """everything the tail calls return on a context, as bytes (pairs in (row, col) order: the order inside a row is open)"""
    from test_gpu_topn_eval import evaluate
    T = rec_sim(ctx, I, U, n_rows)
    o = np.lexsort((T["col"], np.repeat(np.arange(I), np.diff(T["row_ptr"]))))
    for k in ("col", "sim", "ls", "nij"):
        T[k] = T[k][o]
    nb = select(ctx, I, 10)
    P = predict(ctx, tu, ti, real, 1.5)
    R = recommend(ctx, queries, 10, 1, 0, 1.5)
    E = evaluate(ctx, held[0], held[1], held[2], 4.0, 10, 0, 0, 1.5, (1, 5, 10), U)
    out = [T[k] for k in sorted(T)] + list(nb) + list(P[:4]) + [np.asarray(P[4])] + list(R[:4]) + [np.asarray(R[4])] + list(E[:4]) + [np.asarray(E[4])]
    return T, [np.asarray(a).tobytes() for a in out]


def test_union_through_the_coarse_abi():
    import torch
    from test_gpu_recsim import _pairs
    from xmap.engine import device, hipabi as abi
    doms = _trained_domains("multi", 2)
    numbers = np.unique(np.concatenate([r.tgt_numbers for r in doms]))
    U, I = doms[0].n_users, len(numbers)
    rng = np.random.default_rng(8)
    srcs, rows, user_maps, item_maps = [Ctx(), Ctx()], [], [], []
    dst, other = Ctx(), Ctx()
    closed = []
    try:
        for c, r in zip(srcs, doms):
            rows.append(generate(c, r))
            user_maps.append(rng.permutation(U).astype(np.int32))            # a union user numbering of its own
            im = np.full(r.n_items, -1, np.int32)
            im[r.n_src_items:] = np.searchsorted(numbers, r.tgt_numbers)
            item_maps.append(im)
        tu, ti = rng.integers(0, U, 500).astype(np.int32), rng.integers(0, I, 500).astype(np.int32)
        real = rng.integers(1, 6, 500).astype(np.float64)
        queries = rng.integers(0, U, 100).astype(np.int32)
        hu, hi = np.unique(np.stack([rng.integers(0, U, 800), rng.integers(0, I, 800)]), axis=1).astype(np.int32)
        held = (hu, hi, rng.integers(1, 6, len(hu)).astype(np.float64))
        src_before = [_tail_answers(c, r.n_items, U, len(rw["user"]), tu, ti + r.n_src_items, real, queries, (hu, hi + r.n_src_items, held[2]))[1]
                      for c, r, rw in zip(srcs, doms, rows)]
        # a context without generated rows is refused, as source and the destination stays empty
        assert _union(dst, [srcs[0], other], user_maps, item_maps, U, I, 1)[0] == abi.ERR_ARG and b"source 1" in dst.lib.xmap_last_error()
        assert dst.lib.xmap_ctx_rec_sim(dst.h, CAP, None) == abi.ERR_ARG
        assert _union(srcs[0], srcs, user_maps, item_maps, U, I, 1)[0] == abi.ERR_ARG               # dst among the sources
        assert _union(dst, srcs, user_maps, item_maps, U, I, 2)[0] == abi.ERR_ARG                   # unknown flag
        bad = [user_maps[0], np.where(np.arange(U) == 3, user_maps[1][4], user_maps[1]).astype(np.int32)]
        assert _union(dst, srcs, bad, item_maps, U, I, 1)[0] == abi.ERR_ARG and b"twice" in dst.lib.xmap_last_error()
        assert dst.lib.xmap_ctx_rec_sim(dst.h, CAP, None) == abi.ERR_ARG                            # a refused union leaves dst as it was
        # ---- the union, plain first: the second call replaces the first
        host = []
        for rw, um, im in zip(rows, user_maps, item_maps):
            off = lambda seg: np.concatenate([[0], np.cumsum(np.bincount(seg, minlength=U))]).astype(np.int64)
            n_t = int(rw["n_target_rows"])                              # the two segments are in user order each
            host.append(Part.of_arrays(rw, off(rw["user"][:n_t]), off(rw["user"][n_t:]), n_t, um, im))
        rc, counts0 = _union(dst, srcs, user_maps, item_maps, U, I, 0)
        assert rc == 0 and counts0 == union_statement(host, U, I, False)[4]
        T0 = rec_sim(dst, I, U, counts0[0])
        want = union_statement(host, U, I, True)
        rc, counts = _union(dst, srcs, user_maps, item_maps, U, I, 1)
        assert rc == 0 and counts == want[4] and 0 < counts[1] and counts[0] < counts0[0]
        assert dst.lib.xmap_ctx_rec_select(dst.h, 10) == abi.ERR_ARG                                # the first union's tail went with it
        T, answers = _tail_answers(dst, I, U, counts[0], tu, ti, real, queries, held)
        assert np.array_equal(T["ptr"], want[0]) and np.array_equal(T["item"], want[1]) and np.array_equal(T["time"], want[3])
        assert np.array_equal(T["rating"].view(np.uint64), want[2].view(np.uint64))
        assert not np.array_equal(T["ptr"], T0["ptr"])
        # ---- the engine route over the same rows: byte for byte
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        parts = []
        for p in host:
            G = device.GenResult()
            G.user, G.item, G.rating, G.time, G.off_t, G.off_m = to(p.user), to(p.item), to(p.rating), to(p.time), to(p.off_t), to(p.off_m)
            G.n_rows, G.n_target_rows = p.n_rows, p.n_target_rows
            parts.append((G, p.user_map, p.item_map, None))
        P = device.Engine.union_profiles(parts, U, I)
        e2 = device.Engine(P)
        S = e2.rec_sim(CAP)
        nb = e2.rec_select(S, 10)
        avg = S.info[:I, 0].contiguous()
        w = to(wtab(1.5, 66))
        plain, decay, status, max_now = e2.predict(P, nb, to(tu), to(ti), avg, w)
        m = e2.mae(status, to(real), plain, decay)
        t_cnt, t_item, t_plain, t_decay, t_stats = e2.topn(P, nb, to(queries), avg, w, 10, 1, False)
        n_rel, users, ecounts = e2.eval_users(to(held[0]), to(held[1]), to(held[2]), 4.0, U, I)
        e_cnt, e_item, _, _, e_stats = e2.topn(P, nb, users, avg, w, 10, 0, False)
        mask, _, agg, cover = e2.topn_eval(to(held[0]), to(held[1]), to(held[2]), 4.0, n_rel, users, e_cnt, e_item, (1, 5, 10), I)
        full = np.zeros(U, np.uint64)
        full[users.cpu().numpy()] = mask.cpu().numpy().view(np.uint64)
        a, b, sim, ls, nij = _pairs(S, I)
        rp = np.concatenate([[0], np.cumsum(np.bincount(a, minlength=I))]).astype(np.int64)
        eng_T = dict(ptr=P.user_ptr.cpu().numpy(), item=P.user_item.cpu().numpy()[:P.nnz], rating=P.user_rating64.cpu().numpy()[:P.nnz],
                     time=P.user_time.cpu().numpy()[:P.nnz], row_ptr=rp, col=b.astype(np.int32), sim=sim, ls=ls, nij=nij.astype(np.int32),
                     avg=avg.cpu().numpy(), norm=S.norm.cpu().numpy())
        eng_out = [eng_T[k] for k in sorted(eng_T)] + [x.cpu().numpy() for x in nb] + [plain.cpu().numpy(), decay.cpu().numpy(), status.cpu().numpy(), m.cpu().numpy()]
        eng_out += [np.asarray(max_now)] + [t_cnt.cpu().numpy(), t_item.cpu().numpy(), t_plain.cpu().numpy(), t_decay.cpu().numpy(), np.asarray(list(t_stats))]
        eng_out += [agg.cpu().numpy(), cover.cpu().numpy(), n_rel.cpu().numpy(), full, np.asarray(list(ecounts) + list(e_stats))]
        assert sorted(eng_T) == sorted(T)
        eng_bytes = [np.asarray(x).tobytes() for x in eng_out]
        assert len(eng_bytes) == len(answers)
        for k, (x, y) in enumerate(zip(eng_bytes, answers)):
            assert x == y, k
        # ---- what a tail-only context refuses
        z, zi, zf = np.zeros(2, np.int64), np.zeros(1, np.int32), np.zeros(1, np.float32)
        assert dst.lib.xmap_ctx_item_sim(dst.h, 0, CAP, None, None) == abi.ERR_ARG
        assert dst.lib.xmap_ctx_extend(dst.h, 5, None, None) == abi.ERR_ARG
        assert dst.lib.xmap_ctx_generate(dst.h, 1, None, None, None, None) == abi.ERR_ARG
        assert dst.lib.xmap_ctx_gen_download(dst.h, None, None, None, None) == abi.ERR_ARG
        assert dst.lib.xmap_ctx_foldin(dst.h, 1, _p(z, C.c_int64), _p(zi, C.c_int32), _p(zf, C.c_float), _p(z, C.c_int64), None) == abi.ERR_ARG
        assert dst.lib.xmap_ctx_foldin_download(dst.h, None, None, None, None) == abi.ERR_ARG
        wt = wtab(0.2, 8)
        assert dst.lib.xmap_ctx_foldin_recommend(dst.h, 1, _p(zi, C.c_int32), 1, 0, 0, _p(wt, C.c_double), 8, _p(zi, C.c_int32), _p(zi, C.c_int32),
                                                 _p(np.zeros(1), C.c_double), _p(np.zeros(1), C.c_double), None) == abi.ERR_ARG
        assert dst.lib.xmap_ctx_foldin_predict(dst.h, 1, _p(zi, C.c_int32), _p(zi, C.c_int32), None, _p(wt, C.c_double), 8, _p(np.zeros(1), C.c_double),
                                               _p(np.zeros(1), C.c_double), _p(zi, C.c_int32), None, None) == abi.ERR_ARG
        assert _tail_answers(dst, I, U, counts[0], tu, ti, real, queries, held)[1] == answers           # still working, the same bytes
        # ---- the sources are unchanged, and may go
        for c, r, rw, before in zip(srcs, doms, rows, src_before):
            assert _tail_answers(c, r.n_items, U, len(rw["user"]), tu, ti + r.n_src_items, real, queries, (hu, hi + r.n_src_items, held[2]))[1] == before
        for c in srcs:
            c.close()
        closed = srcs
        assert _tail_answers(dst, I, U, counts[0], tu, ti, real, queries, held)[1] == answers
        # ---- an upload drops the union
        from test_gpu_coarse_oracle import upload
        upload(dst, doms[0])
        assert dst.lib.xmap_ctx_rec_sim(dst.h, CAP, None) == abi.ERR_ARG
    finally:
        for c in srcs + [dst, other]:
            if c not in closed:
                c.close()
