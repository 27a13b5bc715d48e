"""tests/quota_statement.py against cases checked by hand, and the census of its designed families: what the device tests
(tests/test_gpu_quota.py) are meant to reach is asserted here as conditions, without a device."""
import numpy as np

import quota_statement as qs
from quota_statement import CAP, SHARE, cap_lists, share_lists


def test_the_hand_checked_cases():
    for L, mode, n_top, rule, positions, claims, third in qs.hand_cases():
        if mode == CAP:
            pos, refused, _ = cap_lists(L, n_top, lambda l: rule)
            assert (pos, refused) == (positions, third)
        else:
            pos, cl, fills, ties = share_lists(L, n_top, rule)
            assert (pos, cl, fills) == (positions, claims, third)
            assert ties >= 1                    # the second slot: 3 / 3 against 1 / 1, label 0 wins


def test_cap_rules_by_hand():
    # a position without governed labels is always accepted; a refused position consumes nothing of its other labels
    L = [[0], [0, 1], [1], [1], []]
    pos, refused, partly = cap_lists(L, 5, lambda l: 1)
    assert (pos, refused, partly) == ([0, 2, 4], 2, 1)          # position 1 refused for label 0 while label 1 had room
    # a barred label; INT32_MAX is no cap
    assert cap_lists(L, 5, lambda l: 0 if l == 0 else qs.INT32_MAX)[0] == [2, 3, 4]
    # the loop stops at n_top: what follows is not refused
    assert cap_lists([[0]] * 6, 2, lambda l: 3)[:2] == ([0, 1], 0)


def test_share_rules_by_hand():
    # all-zero weights: the pool's prefix, every slot a fill
    L = [[0], [1], [0, 2]]
    assert share_lists(L, 2, {}) == ([0, 1], [-1, -1], 2, 0)
    # a label without a position left leaves E; the rest is filled in pool order
    pos, claims, fills, _ = share_lists([[1], [0], [1], []], 4, {0: 5})
    assert (pos, claims, fills) == ([1, 0, 2, 3], [0, -1, -1, -1], 3)
    # a position seated for one label counts for all its labels
    pos, claims, _, _ = share_lists([[0, 1], [1], [0]], 3, {0: 2, 1: 2})
    assert (pos, claims) == ([0, 2, 1], [0, 0, 1])              # after slot 0 both have one seat: 2 / 3 = 2 / 3, label 0 wins


def test_history_weights_and_pool_by_hand():
    labels = qs.Labels.of([[0], [0, 1], [], [2]], 3)
    ok = np.asarray([1, 1, 0], bool)
    assert qs.history_weights(labels, ok, [1, 1, 0, 3, -1, 4, 2]) == {0: 3, 1: 2}
    kept = [(5, 0.0, 1.0), (2, -0.0, 2.0), (9, 1.5, 0.5), (1, -3.0, 2.0)]
    assert [c[0] for c in qs.pool_of(kept, 0, 3)] == [9, 2, 5]          # -0.0 equals 0.0: the item decides
    assert [c[0] for c in qs.pool_of(kept, 1, 4)] == [1, 2, 5, 9]


def test_the_products_need_64_bits():
    """w = {0: 2^31 - 1, 1: 2^30 + 7} over 40 alternating single-label positions: 32-bit products pick another list"""
    L = qs.alternating()
    wide, narrow = share_lists(L, len(L), qs.W32, 64), share_lists(L, len(L), qs.W32, 32)
    assert wide[0] != narrow[0]
    assert max(w * (2 * 20 + 1) for w in qs.W32.values()) >= 1 << 32
    assert sorted(wide[0]) == list(range(40)) and wide[2] == 0


def test_the_census_of_the_designed_families():
    cz = qs.census()
    print(cz)
    assert cz["differs"] > 0                    # a list that differs from the pool's prefix
    assert cz["partly"] > 0                     # refused for one full label while another of its labels still has room
    assert cz["barred"] >= 1                    # a barred label (cap 0)
    assert cz["short_full"] > 0 and cz["short_not_full"] > 0
    assert cz["ties"] > 0                       # a quotient tie decided by label id
    assert cz["fills"] > 0                      # a SHARE fill slot
    assert cz["w32_lists_differ"]
    assert cz["user_holds_item_twice"] and cz["pool_holds_item_twice"]
    assert cz["items_outside"] == [-1, qs.N_ITEMS]
    assert cz["top_label"] == (1 << 24) - 1
    assert cz["records_at_1024"] == qs.MAX_RECORDS and cz["longest_row"] == 8


def test_to_arrays_pads_as_the_header_says():
    lists = [[(2, 40, 1.5, -0.0, 7)], []]
    cnt, item, plain, decay, pos, label = qs.to_arrays(lists, 2)
    assert cnt.tolist() == [1, 0] and item.tolist() == [[40, -1], [-1, -1]] and pos.tolist() == [[2, -1], [-1, -1]]
    assert label.tolist() == [[7, -1], [-1, -1]] and plain.tolist() == [[1.5, 0.0], [0.0, 0.0]]
    assert np.signbit(decay[0, 0]) and not np.signbit(decay[0, 1])
