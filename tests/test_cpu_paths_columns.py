"""A census on the path kernel's side (no GPU needed): the designed families of tests/paths_families.py reach every shape class
of k_paths4 (csrc/paths4.hip), with the counts written next to the inputs, and the statement that counts them
(tests/paths_statement.py) agrees with the independent per-path oracle before any GPU is involved; plan_statement (the
statement of xmap_path_plan) on designed path counts.  tests/test_gpu_paths_columns.py runs the same inputs on the device.

What the generated inputs of the suite reach, for comparison: column_census of three SWEEP_B entries (test_gpu_parity.py),
cosine | adjusted cosine, from the oracle's knn tables (xo.extend(..., do_paths=False)); the statement's n_paths equals the
oracle's recorded path counts on all six (test_generated_inputs_census holds the figures marked *).  The census counts the
starts that have paths: "most heads of a start" leaves out items with more heads and no path.

  quantity                                  s204 (k = 6)         s205 (k = 100)      s207 (k = 64)
  visits                                    156 376 | 144 065    38 834 | 32 571     58 190 | 52 236
  widest column (ends) *                    7 | 7                49 | 45             41 | 38
  visits of a column of > 64 ends *         0 | 0                0 | 0               0 | 0
  ne = 16 | 17 (visits)                     0, 0 | 0, 0          229, 647 | 623, 421 600, 0 | 288, 284
  ne = 32 | 33                              0, 0 | 0, 0          0, 0 | 0, 0         301, 0 | 0, 0
  ne = 64 | 65, ne = k + 1 above 64         0                    0                   0
  R > 64 on a column of 33 .. 64 ends       0 | 0                95 | 39             396 | 173
  most records in a visit                   756 | 619            350 | 353           1 006 | 884
  one head alone with > 64 records          0 | 0                0 | 0               0 | 0
  most heads of a start with paths *        185 | 168            85 | 83             99 | 97
  starts with exactly 64, 65, 128, 129 heads   0                 0                   0
  batches after the first, with a column *  6 | 5                1 | 1               2 | 2
  batches after the first without a column  0 | 0                0 | 0               0 | 0
  late_home_own (visits)                    1 577 | 1 260        88 | 89             208 | 194
  a batch of 17 | 64 heads whose last lane alone holds a column   0, 0 everywhere

No generated input below full size runs the second chunk of a column's ends or a column of 33, 64 or 65 ends, none has a start
on either side of 64 or 128 heads, and a later batch is met by a handful of starts.
"""
import numpy as np
import pytest

from paths_families import BUILDERS, CENSUS, HEAVY, MAX_PATHS, MUST_NE, MUST_PR, MUST_R, PATHS, family_case
from paths_statement import column_census, plan_statement, range_census, statement
from test_cpu_fed_sim import fast_div_ok

FAMILIES = list(BUILDERS)

# (seed, method): paths (the oracle's count recorded at SWEEP_B), widest column, most heads of a start with paths, later
# batches with a column
GENERATED = {(204, "cosine"): (13565319, 7, 185, 6), (204, "adjust_cosine"): (9364396, 7, 168, 5),
             (205, "cosine"): (7288193, 49, 85, 1), (205, "adjust_cosine"): (5260779, 45, 83, 1),
             (207, "cosine"): (26857963, 41, 99, 2), (207, "adjust_cosine"): (19783497, 38, 97, 2)}


@pytest.mark.parametrize("seed,method", list(GENERATED), ids=lambda v: str(v))
def test_generated_inputs_census(seed, method):
    """the statement on generated ratings, from the knn tables alone (no path is enumerated): its path count is the one the
    oracle's enumeration recorded, and what these inputs do not reach is what the docstring's table says"""
    from oracle import xmap_oracle as xo
    from golden_util import CAP
    from test_gpu_parity import SWEEP_B, sweep_ratings
    cfg, = [c for c in SWEEP_B if c["seed"] == seed]
    r = sweep_ratings(cfg)
    attrs = r.item_attrs()
    T = xo.Train(r.user_ptr, r.item, r.rating, r.time, r.n_items, *attrs)
    So = xo.item_sim(T, method, CAP, nthreads=8)
    X = xo.extend(T, So, cfg["k"], do_paths=False)
    St = statement(X.cls, X.cnt, X.col, attrs[3])
    c = column_census(St)
    assert (St.n_paths, c["max_ne"], c["max_nH"], c["later_batches"] - c["later_empty"]) == GENERATED[(seed, method)]
    assert c["ne>64"] == 0 and c["ne=33"] == c["ne=64"] == c["ne=65"] == 0 and c["head>64"] == 0
    assert c["last_lane@17"] == c["last_lane@64"] == 0 and all(c["nH=%d" % n] == 0 for n in (64, 65, 128, 129))
    xo.ext_free(X)
    xo.sim_free(So)


@pytest.mark.parametrize("name", FAMILIES)
def test_family_census(name):
    """the classes a family is designed to reach, with the written counts (every quantity not written is zero)"""
    c = family_case(name)
    got = {q: v for q, v in c.census.items() if v}
    assert got == CENSUS[name]
    V = c.St.visits
    for ne in MUST_NE.get(name, []):
        assert (V[:, 4] == ne).any(), "no column of %d ends" % ne
    for R in MUST_R.get(name, []):
        assert (V[:, 5] == R).any(), "no visit of %d records" % R
    for p, R in MUST_PR.get(name, []):
        assert ((V[:, 6] == p) & (V[:, 5] == R)).any(), "no visit of %d heads with %d records" % (p, R)
    if name == "wide":
        assert V[:, 5].max() <= 16 and c.census["max_nH"] <= 4            # few heads, at most one group of records
        assert (c.Xo.cnt[:, 1] == c.k).sum() == 2                         # k + 1 ends: a full list, and one the list cuts
    if name == "records":
        # 10 + 10: the second of two heads straddles the first group edge
        assert ((V[:, 6] == 2) & (V[:, 5] == 20) & (V[:, 7] == 10) & (V[:, 8] == 1)).any()
        # a second round on a home end of the first batch (what `la = a` in heads_Q is for)
        assert ((V[:, 1] == 0) & (V[:, 5] > 64)).sum() >= 50
    if name == "heads":
        assert c.census["late_home"] >= 100 and c.census["late_home_own"] >= 100


@pytest.mark.parametrize("name", FAMILIES)
def test_statement_against_the_oracle(name):
    """the statement's path count and candidate counts are the per-path oracle's; the family stays under the path bound, on
    the fast division, and the oracle classifies it as designed"""
    c = family_case(name)
    St, Xo, ix = c.St, c.Xo, c.D.ix
    assert St.n_paths == Xo.n_paths == PATHS[name] <= MAX_PATHS
    assert np.array_equal(np.diff(Xo.xs_ptr), St.n_cand)
    assert int((St.n_cand > 0).sum()) >= 3 and St.n_cand.max() > 10          # a list the fused top-10 cuts
    assert St.n_updates < St.n_paths
    assert fast_div_ok(c.sim, c.mutu) == 1
    bridge = np.concatenate([ix["s"], ix["t"]])
    assert np.array_equal(np.nonzero(Xo.cls == 1)[0], np.sort(bridge))
    for g, idx in ix.items():
        if g == "F":
            assert (Xo.cls[idx] == 0).all()             # fillers: dropped by the classification, ends all the same
            assert (St.home[idx] >= 0).any()
        elif g not in ("s", "t"):
            assert (Xo.cls[idx] == 2).all(), g
    if c.starts is not None:
        assert (St.n_cand[:c.start_range[0]] == 0).all() and St.P[:c.start_range[0]].sum() > 0      # the cut removes work


@pytest.mark.parametrize("name", FAMILIES)
def test_matrix_is_symmetric(name):
    c = family_case(name)
    rows = np.repeat(np.arange(c.I), np.diff(c.row_ptr))
    assert np.all(np.diff(c.row_ptr) > 0) and len(rows) == 2 * len(c.D.edges)
    back = {(int(a), int(b)): (s.tobytes(), int(m)) for a, b, s, m in zip(rows, c.col, c.sim, c.mutu)}
    assert all(back[(b, a)] == v for (a, b), v in back.items())
    assert np.array_equal(c.nij, c.mutu) and c.mutu.min() >= 1 and c.mutu.max() <= 7
    assert 0.05 <= np.abs(c.sim).min() and np.abs(c.sim).max() <= 0.95 and (c.sim < 0).any() and (c.sim > 0).any()


@pytest.mark.parametrize("name", FAMILIES)
def test_statement_does_not_depend_on_the_listing_order(name):
    """the pairs of every row listed in descending and in shuffled order: the oracle's tables, hence the statement, are the same
    (the statement reads the classified tables alone and orders its lists by item)"""
    from oracle import xmap_oracle as xo
    c = family_case(name)
    for order in ("desc", 7):
        row_ptr, col, sim, mutu, nij, info = c.D.arrays(c.seed, order=order)
        assert np.array_equal(row_ptr, c.row_ptr) and not np.array_equal(col, c.col)
        So = xo.sim_from_arrays(c.I, row_ptr, col, sim, mutu, nij, info)
        X = xo.extend(c.T, So, c.k, do_paths=False)
        held = np.arange(c.k)[None, None, :] < c.Xo.cnt[:, :, None]
        assert np.array_equal(X.cls, c.Xo.cls) and np.array_equal(X.cnt, c.Xo.cnt) and np.array_equal(X.col[held], c.Xo.col[held])
        St = statement(X.cls, X.cnt, X.col, c.attrs[3], starts=c.starts)
        assert np.array_equal(St.visits, c.St.visits) and np.array_equal(St.P, c.St.P)
        assert (St.n_paths, St.n_updates, St.n_tiles, St.n_records) == (c.St.n_paths, c.St.n_updates, c.St.n_tiles, c.St.n_records)
        assert column_census(St) == c.census
        xo.ext_free(X)
        xo.sim_free(So)


@pytest.mark.parametrize("form", HEAVY, ids=lambda f: "%s-%d" % (f[0], f[1]))
def test_heavy_forms(form):
    """the written chunk values cut the starts as written: G on both sides of MERGE_GROUP, RX = 1 and RX > 1, columns beyond
    the first range"""
    name, chunk, n_slots, want, h_out = form
    c = family_case(name)
    lo, hi = c.start_range or (0, c.I)
    pl = plan_statement(c.St.P, lo, hi, chunk, 0, 1 << 40)
    assert pl["h_out"] == h_out
    assert range_census(c.St, pl["G"]) == want
    assert h_out[3] == c.St.n_paths


def test_heavy_forms_cover():
    G = set(g for f in HEAVY for g in f[3]["G"])
    assert {2, 12, 13, 24, 25} <= G
    assert sum(f[3]["rx1"] for f in HEAVY) >= 1 and sum(f[3]["rx>1"] for f in HEAVY) >= 1
    assert sum(f[3]["hi_range"] for f in HEAVY) >= 10 and sum(f[3]["odd_group"] for f in HEAVY) >= 2
    deep = {g: f[3]["deep_rows"] for f in HEAVY for g in f[3]["G"] if g > 12 and f[3]["deep_rows"]}
    assert deep.get(13, 0) >= 1 and deep.get(25, 0) >= 13      # sums in the rows that only the second merge level reaches
    assert {f[2] for f in HEAVY} == {1, 3, 64} and {f[0] for f in HEAVY} == {"records", "heads"}


# ---- plan_statement on designed path counts (no graph needed) ---------------------------------------------------------------
# (name, P, lo, hi, chunk, chunk_div, max_rows, h_out, unit_G in unit order or None)
C = 100
PLANS = [
    ("around the chunk", [0, 1, C, C + 1, 2 * C, 2 * C + 1, 0, 5], 0, 8, C, 0, 1 << 20, [10, 3, 7, 608, C],
     [1, 2, 2, 3, 3, 3, 2, 2, 1, 1]),
    ("equal costs", [7, 300, 7, 150, 7, 300, 150, 7], 0, 8, C, 0, 1 << 20, [14, 4, 10, 928, C], None),
    ("above 2^44", [1 << 45, 3, (1 << 44) + 5, 1 << 46, 9], 0, 5, 1 << 47, 0, 1 << 20, [5, 0, 0, (1 << 45) + (1 << 44) + (1 << 46) + 17, 1 << 47],
     [1, 1, 1, 1, 1]),
    ("a start range", [500, 40, 250, 0, 999, 60, 700], 2, 6, C, 0, 1 << 20, [14, 2, 13, 1309, C], None),
    ("max_rows = 2", [1000, 500, 50, 3], 0, 4, 10, 0, 2, [5, 1, 2, 1553, 640], None),
    ("no budget at all", [1000, 900, 50, 3], 0, 4, 10, 0, -1, [4, 0, 0, 1953, 2560], None),
    ("chunk_div below 2^22", [1 << 21, 1 << 23, 5], 0, 3, 0, 8192, 1 << 20, [4, 1, 2, (1 << 21) + (1 << 23) + 5, 1 << 22], None),
    ("chunk_div above 2^22", [1 << 36, 1 << 20, 3 << 34], 0, 3, 0, 1 << 10, 1 << 20, None, None),
    ("one item", [12345], 0, 1, C, 0, 1 << 20, [124, 1, 124, 12345, C], None),
    ("all zero", [0] * 9, 0, 9, C, 0, 1 << 20, [0, 0, 0, 0, C], None),
    ("all zero, chunk_div", [0] * 9, 0, 9, 0, 8192, 1 << 20, [0, 0, 0, 0, 1 << 22], None),
]


@pytest.mark.parametrize("plan", PLANS, ids=[p[0] for p in PLANS])
def test_plan_statement(plan):
    name, P, lo, hi, chunk, div, max_rows, h_out, unit_G = plan
    pl = plan_statement(P, lo, hi, chunk, div, max_rows)
    P = np.asarray(P, np.int64)
    if h_out is not None:
        assert pl["h_out"] == h_out
    n_units, n_heavy, n_rows, total, ch = pl["h_out"]
    us, uc, ug, ur, h0, G = (pl[n] for n in ("unit_start", "unit_c", "unit_G", "unit_row", "heavy_unit0", "G"))
    if unit_G is not None:
        assert ug.tolist() == unit_G
    # the properties the kernels rely on, whatever the numbers
    inside = (np.arange(len(P)) >= lo) & (np.arange(len(P)) < hi) & (P > 0)
    assert total == int(P[inside].sum()) and n_units == int(G.sum()) == len(us)
    assert sorted(set(us.tolist())) == np.nonzero(inside)[0].tolist()
    assert np.array_equal(G[inside], np.where(P[inside] > ch, -(-P[inside] // ch), 1))
    assert n_heavy == int((G > 1).sum()) == len(h0) and n_rows == int(G[G > 1].sum())
    cost = np.minimum(P[us] // ug, (1 << 44) - 1)
    assert np.all(np.diff(cost) <= 0)                                        # heaviest unit first
    for a, b in zip(range(len(us) - 1), range(1, len(us))):
        if cost[a] == cost[b] and us[a] != us[b]:
            assert us[a] < us[b]                                             # equal costs in start order
    for u0 in h0:
        g = ug[u0]
        assert (us[u0:u0 + g] == us[u0]).all() and uc[u0:u0 + g].tolist() == list(range(g))
        assert ur[u0:u0 + g].tolist() == list(range(ur[u0], ur[u0] + g))     # consecutive rows: what k_merge adds up
    assert sorted(ur[ur >= 0].tolist()) == list(range(n_rows)) and (ur[ug == 1] == -1).all()
    if name == "above 2^44":
        assert us.tolist() == [0, 2, 3, 4, 1]                # the three capped costs tie: start order
    if name == "equal costs":
        assert us.tolist() == [1, 1, 1, 5, 5, 5, 3, 3, 6, 6, 0, 2, 4, 7]
    if name == "max_rows = 2":
        assert ch == 10 << 6                                 # six doublings: 1 000 paths leave two rows at a chunk of 640
    if name == "no budget at all":
        assert ch > total and ch // 2 <= total               # the exit `chunk > total`
    if name == "chunk_div above 2^22":
        assert ch == total // (1 << 10) > 1 << 22 and n_heavy == 2
