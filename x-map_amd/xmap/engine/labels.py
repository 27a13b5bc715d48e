"""Host helpers for the shelves and the quotas (xmap_shelf_rows / xmap_quota_rows / xmap_ctx_set_labels of include/xmap_hip.h): the
label table of an item space as the CSR the device calls read, the bitmap of the labels that may form a shelf or that a quota
governs, and the per-label caps / weights of a quota call.  NumPy only."""
import numpy as np

from .filters import pack_mask

MAX_LABELS = 1 << 24        # XMAP_SHELF_MAX_LABELS


def label_csr(per_item_labels, n_items):
    """The label table of an item space of n_items items as (n_labels, lab_ptr int64 [n_items + 1], lab_id int32, names).
    per_item_labels: {item index: labels} or a sequence with one entry of labels per item (None or empty: no label); a label is
    any sortable hashable value (a name).  names = the distinct labels in sorted order, label id = position in names.  Per item
    the ids are sorted and a repeated label stands once, as the device contract asks.  An item index outside [0, n_items) is
    ignored (an item the model does not know)."""
    n_items = int(n_items)
    if n_items < 0:
        raise ValueError("label_csr: n_items = %d" % n_items)
    if isinstance(per_item_labels, dict):
        rows = [()] * n_items
        for i, l in per_item_labels.items():
            if 0 <= int(i) < n_items and l is not None:
                rows[int(i)] = tuple(l)
    else:
        rows = [() if l is None else tuple(l) for l in per_item_labels]
        if len(rows) != n_items:
            raise ValueError("label_csr: %d rows of labels for %d items" % (len(rows), n_items))
    names = sorted({x for r in rows for x in r})
    if len(names) > MAX_LABELS:
        raise ValueError("label_csr: %d labels, the table takes %d" % (len(names), MAX_LABELS))
    at = {x: k for k, x in enumerate(names)}
    ids = [sorted({at[x] for x in r}) for r in rows]
    lab_ptr = np.zeros(n_items + 1, np.int64)
    if n_items:
        np.cumsum([len(r) for r in ids], out=lab_ptr[1:])
    lab_id = np.asarray([k for r in ids for k in r], np.int32)
    return len(names), lab_ptr, lab_id, names


def label_mask(names, chosen):
    """The `lab_allow` words over the labels `names` (label_csr's): bit (l & 31) of word (l >> 5) set for the labels of `chosen`
    (names, any order, repeats allowed).  A name that is no label raises: a misspelt category would silently empty the page."""
    at = {x: k for k, x in enumerate(names)}
    missing = [x for x in chosen if x not in at]
    if missing:
        raise ValueError("label_mask: %r is no label of the table" % (missing[0],))
    return pack_mask(np.asarray(sorted({at[x] for x in chosen}), np.int64), len(names))


def label_values(names, mapping, default, dtype):
    """The per-label array of a quota call (`lab_cap` int32, `lab_weight` uint32) over the labels `names` (label_csr's): the value
    of `mapping` {label name: value} where it names the label, `default` elsewhere.  A name that is no label raises, as in
    label_mask; a value the dtype does not hold raises too (a negative weight, a cap above INT32_MAX)."""
    at = {x: k for k, x in enumerate(names)}
    missing = [x for x in mapping if x not in at]
    if missing:
        raise ValueError("label_values: %r is no label of the table" % (missing[0],))
    info = np.iinfo(dtype)
    out = np.empty(len(names), dtype)
    for k, x in enumerate(names):
        v = int(mapping.get(x, default))
        if not info.min <= v <= info.max:
            raise ValueError("label_values: %r = %d does not fit %s" % (x, v, np.dtype(dtype).name))
        out[k] = v
    return out
