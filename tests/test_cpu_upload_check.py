"""xmap_check_ratings, the host-side check both front doors run before anything reaches the device (xmap_ctx_upload_ratings:
XMAP_ERR_ARG; DeviceRatings: ValueError with the same text): what it refuses, the position it names, what it lets pass.  Host
code only -- no context, no device.  (The coarse door's use of it: tests/test_gpu_coarse_oracle.py.)"""
import ctypes
import re

import numpy as np
import pytest

I, N_SRC = 9, 5


def good():
    """4 users (the third without ratings) over 9 items: (user_ptr, item, prefix_cls, suffix_cls)"""
    ptr = np.asarray([0, 3, 5, 5, 9], np.int64)
    item = np.asarray([0, 4, 7, 2, 8, 8, 1, 0, 5], np.int32)
    cls = (np.arange(I) >= N_SRC).astype(np.int32)
    return ptr, item, cls.copy(), cls.copy()


def check(ptr, item, pre, suf, allow_repeats=0, n_items=I):
    from xmap.engine import hipabi
    p = lambda a: None if a is None else a.ctypes.data
    rc = hipabi.lib.xmap_check_ratings(len(ptr) - 1, n_items, p(ptr), p(item), p(pre), p(suf), allow_repeats)
    return rc, (hipabi.lib.xmap_last_error() or b"").decode()


def test_the_check_is_declared_exported_and_typed():
    from xmap.engine import hipabi
    v, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert "xmap_check_ratings" in hipabi.EXPORTS
    assert hipabi.PROTOTYPES["xmap_check_ratings"] == [i64, i32, v, v, v, v, i32]
    assert list(hipabi.lib.xmap_check_ratings.argtypes) == hipabi.PROTOTYPES["xmap_check_ratings"]
    assert hasattr(hipabi.xlib(), "xmap_check_ratings")
    assert hipabi.lib.xmap_version() >= 106


def test_legal_uploads_pass():
    ptr, item, pre, suf = good()
    assert check(ptr, item, pre, suf)[0] == 0
    assert check(ptr, item, None, None)[0] == 0                                  # predicate arrays not given: not checked
    suf[3], pre[3] = 31, 2 ** 31 - 1                                             # the largest legal classes
    assert check(ptr, item, pre, suf)[0] == 0
    z = np.zeros(1, np.int64)
    assert check(z, None, None, None, n_items=0)[0] == 0                         # no users, no items
    assert check(np.zeros(4, np.int64), None, pre, suf)[0] == 0                  # users without a rating only
    cls = np.zeros(I + 1000, np.int32)
    assert check(ptr, item, cls, cls, n_items=I + 1000)[0] == 0                  # a thousand unrated items behind


CASES = [
    # (what to break, expected text)
    ("ptr0", r"user_ptr\[0\] = 2, not 0"),
    ("ptr_decreases", r"user_ptr\[3\] < user_ptr\[2\]"),
    ("ptr_decreases_twice", r"user_ptr\[2\] < user_ptr\[1\]"),
    ("item_negative", r"item\[6\] = -1 outside \[0, 9\)"),
    ("item_too_large", r"item\[4\] = 9 outside \[0, 9\)"),
    ("repeat", r"user 3 holds item 8 twice \(item\[5\] and item\[8\]\)"),
    ("repeat_adjacent", r"user 0 holds item 4 twice \(item\[1\] and item\[2\]\)"),
    ("suffix_32", r"suffix_cls\[6\] = 32 outside \[0, 32\)"),
    ("suffix_negative", r"suffix_cls\[0\] = -1 outside \[0, 32\)"),
    ("prefix_negative", r"prefix_cls\[8\] = -5 is negative"),
]


def broken(kind):
    ptr, item, pre, suf = good()
    if kind == "ptr0":
        ptr[0] = 2
    elif kind == "ptr_decreases":
        ptr[3] = 4                              # 0 3 5 4 9: the lengths still sum to nnz
    elif kind == "ptr_decreases_twice":
        ptr[2], ptr[3] = 2, 1                   # the FIRST offending position is named
    elif kind == "item_negative":
        item[6] = -1
    elif kind == "item_too_large":
        item[4], item[7] = 9, 12
    elif kind == "repeat":
        item[8] = 8                             # user 3: 8 1 0 8
    elif kind == "repeat_adjacent":
        item[2] = 4
    elif kind == "suffix_32":
        suf[6], suf[7] = 32, 40
    elif kind == "suffix_negative":
        suf[0] = -1
    elif kind == "prefix_negative":
        pre[8] = -5
    return ptr, item, pre, suf


@pytest.mark.parametrize("kind,text", CASES, ids=[c[0] for c in CASES])
def test_bad_uploads_are_refused_naming_the_position(kind, text):
    from xmap.engine import hipabi
    rc, msg = check(*broken(kind))
    assert rc == hipabi.ERR_ARG, msg
    assert re.search(text, msg), msg


def test_an_item_of_two_users_is_no_repeat_and_alterego_profiles_may_repeat():
    """the stamp of an item belongs to one profile: the same item in the next user's profile passes, also at the first
    position of that profile; allow_repeats (RecommenderSim's AlterEgo profiles) lets a repeat pass and nothing else"""
    from xmap.engine import hipabi
    ptr, item, pre, suf = good()
    item[3] = 7                                                          # users 0 and 1 both hold 7; user 1 starts with it
    item[5] = 0                                                          # user 3 starts with user 0's first item
    item[7] = 4
    assert check(ptr, item, pre, suf)[0] == 0
    rep = broken("repeat")
    assert check(*rep, allow_repeats=1)[0] == 0
    for kind, text in CASES:
        if not kind.startswith("repeat"):
            rc, msg = check(*broken(kind), allow_repeats=1)
            assert rc == hipabi.ERR_ARG and re.search(text, msg), (kind, msg)


def test_the_golden_inputs_and_the_generator_pass():
    """no committed input holds what the check refuses"""
    from golden_util import CASES as GOLDEN, Golden
    from xmap.engine import synth
    for name in GOLDEN:
        g = Golden(name)
        ptr, item = np.ascontiguousarray(g.ptr, np.int64), np.ascontiguousarray(g.item, np.int32)
        pre, suf = [np.ascontiguousarray(a, np.int32) for a in g.attrs[:2]]
        rc, msg = check(ptr, item, pre, suf, n_items=g.I)
        assert rc == 0, (name, msg)
    r = synth.make_two_domain(3, 400, 90, 90)
    pre, suf = [np.ascontiguousarray(a, np.int32) for a in r.item_attrs()[:2]]
    assert check(r.user_ptr, r.item, pre, suf, n_items=r.n_items)[0] == 0


@pytest.mark.parametrize("kind,text", CASES, ids=[c[0] for c in CASES])
def test_device_ratings_raises_with_the_same_text_before_any_upload(kind, text):
    """the engine's door: ValueError with the check's text, raised before a tensor is made (so: without a device)"""
    from xmap.engine import device
    ptr, item, pre, suf = broken(kind)
    attrs = (pre, suf, np.ones(I, np.uint32), np.ones(I, np.uint8))
    with pytest.raises(ValueError, match=text):
        device.DeviceRatings(ptr, item, np.ones(len(item), np.float32), np.zeros(len(item), np.int64), I, attrs, device="cuda:0")
