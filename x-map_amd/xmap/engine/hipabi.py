"""ctypes binding of libxmap_hip.so (C ABI declared in include/xmap_hip.h).

The product path has NO CPU fallback: if the HIP library is missing, import of this
module raises (build it with `python -c "import __graft_entry__ as g; g.build()"` or
`make -C x-map_amd/csrc`).
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("XMAP_HIP_LIB") or os.path.normpath(os.path.join(HERE, "..", "..", "libxmap_hip.so"))
# the same sources + the TEST formulations (-DXMAP_CROSSCHECK): loaded on demand by xlib(), by tests and tuning tools only
XLIB_PATH = os.environ.get("XMAP_HIP_XLIB") or os.path.normpath(os.path.join(HERE, "..", "..", "libxmap_hip_xcheck.so"))

COSINE, ADJUST_COSINE = 0, 1
METHODS = {"cosine": COSINE, "adjust_cosine": ADJUST_COSINE}
COSINE_EXACT = 2          # XMAP_COSINE_EXACT: cosine with double-double sums (the pair entry points only)
TOPC = 10
MID_ROWS_SPAN = 36864     # XMAP_MID_ROWS_SPAN: columns of a middle-list row per LDS pass
ERR_HIP, ERR_ARG, ERR_OVERFLOW, ERR_CAPACITY = -1, -2, -3, -4     # XMAP_ERR_* of include/xmap_hip.h
TOPN_KEEP_HELD = 1        # XMAP_TOPN_KEEP_HELD: flag of xmap_topn_rows / xmap_ctx_recommend
AUDIENCE_KEEP_HOLDERS = 1 # XMAP_AUDIENCE_KEEP_HOLDERS: flag of xmap_audience_rows / xmap_ctx_audience
SRC_RESIDENT, SRC_FOLDIN, SRC_ITEM_FOLDIN = 0, 1, 2      # XMAP_SRC_*: source of xmap_ctx_recommend_filtered / xmap_ctx_audience_filtered
GROUP_MEAN, GROUP_MIN, GROUP_MAX = 0, 1, 2      # XMAP_GROUP_*: `how` of xmap_group_topn_rows / xmap_ctx_recommend_group
GROUP_MAX_MEMBERS = 64    # XMAP_GROUP_MAX_MEMBERS: members of one group
PEERS_SAME, PEERS_KEEP_SELF, PEERS_CENTRED = 1, 2, 4      # XMAP_PEERS_*: flags of xmap_peer_rows / xmap_ctx_peers
UKNN_OWN_MEAN, UKNN_KEEP_HELD = 1, 2      # XMAP_UKNN_*: flags of xmap_uknn_predict_rows / xmap_uknn_topn_rows and the coarse calls
RELATED_SUM, RELATED_MEAN, RELATED_MAX = 0, 1, 2      # XMAP_RELATED_*: `how` of xmap_related_rows / xmap_ctx_related
RELATED_KEEP_MEMBERS = 1  # XMAP_RELATED_KEEP_MEMBERS: flag of the same
RELATED_HOW = {"sum": RELATED_SUM, "mean": RELATED_MEAN, "max": RELATED_MAX}
POP_COUNT, POP_MEAN = 0, 1      # XMAP_POP_*: `how` of xmap_pop_index / xmap_ctx_popular / xmap_ctx_recommend_filled
FILL_WINDOW = 4096        # XMAP_FILL_WINDOW: rank positions one wave of xmap_topn_fill_rows marks at a time
POP_HOW = {"count": POP_COUNT, "mean": POP_MEAN}
FUSE_RRF, FUSE_SUM, FUSE_MEAN = 0, 1, 2      # XMAP_FUSE_*: `how` of xmap_fuse_rows / xmap_ctx_fuse / xmap_ctx_recommend_hybrid
FUSE_MAX_LISTS = 16       # XMAP_FUSE_MAX_LISTS: lists of one fuse
FUSE_BLOCK_RECORDS = 2048 # XMAP_FUSE_BLOCK_RECORDS: the sum of the widths up to which one workgroup fuses a query in LDS
FUSE_HOW = {"rrf": FUSE_RRF, "sum": FUSE_SUM, "mean": FUSE_MEAN}
SHELF_BY_BEST, SHELF_BY_MEAN, SHELF_BY_LABEL = 0, 1, 2      # XMAP_SHELF_BY_*: `shelf_by` of xmap_shelf_rows / xmap_shelf_segments / xmap_ctx_recommend_shelves
SHELF_MAX_LABELS = 1 << 24  # XMAP_SHELF_MAX_LABELS: labels of one table
QUOTA_CAP, QUOTA_SHARE = 0, 1      # XMAP_QUOTA_*: `mode` of xmap_quota_pool / xmap_quota_rows / xmap_ctx_recommend_quota
QUOTA_MAX_POOL = 1024     # XMAP_QUOTA_MAX_POOL: positions of one pool
QUOTA_MAX_RECORDS = 8192  # XMAP_QUOTA_MAX_RECORDS: n_pool x the longest label row of the table
ALLOT_MAX_POOL = 1024     # XMAP_ALLOT_MAX_POOL: positions of one pool of xmap_allot_pool (xmap_allot_rows / xmap_ctx_recommend_allot: 64)
GROUP_HOW = {"mean": GROUP_MEAN, "min": GROUP_MIN, "max": GROUP_MAX}
UNION_DISTINCT = 1        # XMAP_UNION_DISTINCT: flag of xmap_union_count / xmap_union_fill / xmap_ctx_union
UNION_MAX_PARTS = 16
EXPLAIN_MAX_EV, EXPLAIN_MAX_SRC = 16, 8      # evidence entries per pair / source positions per entry of xmap_explain_*
# phases of xmap_sim2_pairs (XMAP_PAIRS_*) and of xmap_sim3_layout (XMAP_LAYOUT_*); tests/test_cpu_host.py holds them to the header
PAIRS_HEAVY, PAIRS_LIGHT, PAIRS_HEAVY_MERGE, PAIRS_RESET = 1, 2, 4, 8
PAIRS_MIRCOUNT, PAIRS_RAW, PAIRS_SHARD_SUMS, PAIRS_NO_MARKS = 16, 32, 64, 128
LAYOUT_RECORDS, LAYOUT_STATS, LAYOUT_UB_FLAGS, LAYOUT_RC_FLAGS, LAYOUT_ALL = 1, 2, 4, 8, 15


def pairs_deal(m, r):
    """XMAP_PAIRS_DEAL: of the heavy rows only those with item index % m == r"""
    return ((int(m) & 0xff) << 16) | ((int(r) & 0xff) << 8)


class XmapError(RuntimeError):
    def __init__(self, code, msg):
        RuntimeError.__init__(self, "libxmap_hip error %d: %s" % (code, msg))
        self.code = code


class Ratings(C.Structure):
    _fields_ = [("n_users", C.c_int64), ("n_items", C.c_int32), ("nnz", C.c_int64),
                ("user_ptr", C.c_void_p), ("user_item", C.c_void_p), ("user_rating", C.c_void_p),
                ("user_time", C.c_void_p), ("item_ptr", C.c_void_p), ("item_user", C.c_void_p),
                ("item_rating", C.c_void_p), ("prefix_cls", C.c_void_p), ("suffix_cls", C.c_void_p),
                ("contains_mask", C.c_void_p), ("flags", C.c_void_p)]


class Sim(C.Structure):
    _fields_ = [("n_items", C.c_int32), ("row_ptr", C.c_void_p), ("col", C.c_void_p), ("sim", C.c_void_p),
                ("mutu", C.c_void_p), ("nij", C.c_void_p), ("info", C.c_void_p), ("frac", C.c_void_p)]


class ExtTables(C.Structure):
    """xmap_ext_tables: the stage-B tables of one pass (device pointers)"""
    _fields_ = [("n_items", C.c_int32), ("top_k", C.c_int32),
                ("cls", C.c_void_p), ("kcnt", C.c_void_p), ("kcol", C.c_void_p), ("kval", C.c_void_p), ("flags", C.c_void_p),
                ("att_ptr", C.c_void_p), ("att_idx", C.c_void_p), ("att_val", C.c_void_p),
                ("src_ptr", C.c_void_p), ("src_idx", C.c_void_p), ("src_val", C.c_void_p), ("src_flag", C.c_void_p),
                ("rnn_ptr", C.c_void_p), ("rnn_idx", C.c_void_p), ("rnn_val", C.c_void_p),
                ("n_nb", C.c_int32), ("nb_id", C.c_void_p), ("nb_list", C.c_void_p), ("midX", C.c_void_p), ("dir", C.c_void_p),
                ("dir_ptr", C.c_void_p),
                ("n_ends", C.c_int32), ("urank", C.c_void_p), ("uitem", C.c_void_p)]


class UnionPart(C.Structure):
    """xmap_union_part: one domain's stage-C rows + its maps into the union's index spaces (device pointers)"""
    _fields_ = [("n_users", C.c_int64), ("n_items", C.c_int32), ("n_rows", C.c_int64), ("n_target_rows", C.c_int64),
                ("user", C.c_void_p), ("item", C.c_void_p), ("rating", C.c_void_p), ("time", C.c_void_p),
                ("off_t", C.c_void_p), ("off_m", C.c_void_p), ("user_map", C.c_void_p), ("item_map", C.c_void_p)]


class PathUnits(C.Structure):
    _fields_ = [("n_units", C.c_int32), ("unit_start", C.c_void_p), ("unit_c", C.c_void_p), ("unit_G", C.c_void_p),
                ("unit_row", C.c_void_p), ("unit_nt", C.c_void_p), ("n_heavy", C.c_int32), ("heavy_unit0", C.c_void_p)]


class PathRows(C.Structure):
    _fields_ = [("n_slots", C.c_int32), ("acc", C.c_void_p), ("touched", C.c_void_p), ("hacc", C.c_void_p),
                ("htouched", C.c_void_p)]


class PathOut(C.Structure):
    _fields_ = [("n_cand", C.c_void_p), ("top_end", C.c_void_p), ("top_val", C.c_void_p), ("xs_cap", C.c_int64),
                ("xs_off", C.c_void_p), ("xs_end", C.c_void_p), ("xs_val", C.c_void_p)]


class RecFilter(C.Structure):
    """xmap_rec_filter: the eligibility rules of a filtered top-N / audience call (device pointers for the fine-grained calls,
    host pointers for the coarse ones); rec_filter() fills one"""
    _fields_ = [("allow", C.c_void_p), ("ex_ptr", C.c_void_p), ("ex_id", C.c_void_p), ("min_score", C.c_double)]


class FuseList(C.Structure):
    """xmap_fuse_list: one list of a fuse (device pointers for xmap_fuse_rows, host pointers for xmap_ctx_fuse)"""
    _fields_ = [("cnt", C.c_void_p), ("item", C.c_void_p), ("score", C.c_void_p), ("width", C.c_int32), ("weight", C.c_double)]


EXPORTS = [
    "xmap_last_error", "xmap_version", "xmap_trim", "xmap_debug_arena", "xmap_debug_arena_call", "xmap_debug_sort_pairs", "xmap_debug_record_chunks", "xmap_exclusive_scan_i64", "xmap_exclusive_scan_i32_to_i64",
    "xmap_exclusive_scan2_i32_to_i64", "xmap_scan_self_tiles", "xmap_sim3_plan_begin", "xmap_sim3_plan_wait", "xmap_sim3_counters_begin", "xmap_sim3_counters_wait",
    "xmap_build_csc", "xmap_user_stats", "xmap_item_stats", 
    "xmap_sim2_layout", "xmap_sim2_plan", "xmap_sim2_units",
    "xmap_sim2_pairs", "xmap_sim2_scatter", "xmap_sim3_layout", "xmap_sim3_plan", "xmap_sim3_mircount", "xmap_sim3_mirror", "xmap_item_partials", "xmap_item_merge", "xmap_sim2_pack_partials",
    "xmap_sim2_sort_partials", "xmap_sim2_merge_partials", "xmap_sim2_pack_pairs", "xmap_sim2_unpack_pairs", "xmap_bridge_flags", "xmap_knn_classify", "xmap_knn_thresholds", "xmap_reverse_count", "xmap_reverse_count_att_rnn",
    "xmap_reverse_fill", "xmap_topc_from_lists", "xmap_path_weights", "xmap_extend_paths", 
    "xmap_mid_rows_count", "xmap_mid_rows_place", "xmap_edge_ranges", "xmap_end_universe", "xmap_extend_cols", "xmap_extend_cols_slots", "xmap_nb_index", "xmap_path_plan", "xmap_end_order", "xmap_dense_normalize", "xmap_dense_layout", "xmap_dense_topk", "xmap_rec_select", "xmap_predict", "xmap_rec_profiles", "xmap_predict_rows", "xmap_mae", "xmap_topn_rows", "xmap_audience_rows", "xmap_explain_rows", "xmap_explain_sources", "xmap_eval_users", "xmap_topn_eval", "xmap_select_map", "xmap_alterego_count", "xmap_alterego_fill", "xmap_foldin_count", "xmap_foldin_fill", "xmap_union_count", "xmap_union_fill",
    "xmap_feed_text", "xmap_feed_texts", "xmap_feed_merge", "xmap_feed_sizes", "xmap_feed_arrays", "xmap_feed_ids", "xmap_feed_free",
    "xmap_ctx_upload_feed", "xmap_feed_format", "xmap_ctx_create", "xmap_ctx_destroy", "xmap_check_ratings", "xmap_ctx_upload_ratings", "xmap_ctx_item_sim", "xmap_ctx_sim_download", "xmap_ctx_extend",
    "xmap_ctx_ext_download", "xmap_ctx_ext_lists", "xmap_ctx_candidates", "xmap_ctx_generate", "xmap_ctx_gen_download",
    "xmap_ctx_rec_sim", "xmap_ctx_rec_profiles_download", "xmap_ctx_rec_download", "xmap_ctx_rec_select", "xmap_ctx_rec_set_neighbors",
    "xmap_ctx_rec_neighbors_download", "xmap_ctx_predict", "xmap_ctx_recommend", "xmap_ctx_evaluate_topn",
    "xmap_ctx_foldin", "xmap_ctx_foldin_download", "xmap_ctx_foldin_recommend", "xmap_ctx_foldin_predict", "xmap_ctx_union",
    "xmap_ctx_explain", "xmap_ctx_foldin_explain", "xmap_ctx_audience", "xmap_ctx_foldin_audience",
    "xmap_itemfold_count", "xmap_itemfold_fill", "xmap_itemfold_audience_rows", "xmap_ctx_item_foldin", "xmap_ctx_item_foldin_download",
    "xmap_ctx_item_foldin_audience", "xmap_ctx_item_foldin_predict", "xmap_ctx_item_foldin_recommend",
    "xmap_topn_rows_filtered", "xmap_audience_rows_filtered", "xmap_ctx_recommend_filtered", "xmap_ctx_audience_filtered",
    "xmap_div_index", "xmap_diversify_rows", "xmap_ctx_recommend_diverse",
    "xmap_group_topn_rows", "xmap_ctx_recommend_group",
    "xmap_peer_index", "xmap_peer_centre", "xmap_peer_rows", "xmap_ctx_peers", "xmap_peer_rows_ls", "xmap_ctx_peers_ls",
    "xmap_uknn_means", "xmap_uknn_predict_rows", "xmap_uknn_topn_rows", "xmap_ctx_uknn_predict", "xmap_ctx_uknn_recommend",
    "xmap_related_rows", "xmap_ctx_related",
    "xmap_pop_index", "xmap_topn_fill_rows", "xmap_ctx_popular", "xmap_ctx_recommend_filled",
    "xmap_fuse_rows", "xmap_ctx_fuse", "xmap_ctx_recommend_hybrid",
    "xmap_shelf_segments", "xmap_shelf_rows", "xmap_ctx_set_labels", "xmap_ctx_recommend_shelves",
    "xmap_quota_pool", "xmap_quota_rows", "xmap_ctx_recommend_quota",
    "xmap_allot_pool", "xmap_allot_rows", "xmap_ctx_recommend_allot",
]

if not os.path.exists(LIB_PATH):
    raise ImportError("libxmap_hip.so not built (%s); the MI355X engine has no CPU fallback" % LIB_PATH)
lib = C.CDLL(LIB_PATH)
lib.xmap_last_error.restype = C.c_char_p
for _n in EXPORTS:
    getattr(lib, _n)  # every symbol the header declares must be exported
# declared under #ifdef XMAP_CROSSCHECK in the header: the test formulations (stage A by complete rows, the round-1 tile-major
# enumeration, the dense-table form of the middle lists) -- exported by libxmap_hip_xcheck.so only
XCHECK_EXPORTS = ["xmap_sim_plan", "xmap_sim_units", "xmap_sim_count", "xmap_sim_fill", "xmap_sim_row_ptr", "xmap_extend_paths2",
                  "xmap_mid_tally", "xmap_mid_place"]

HEADER_PATH = os.path.normpath(os.path.join(HERE, "..", "..", "..", "include", "xmap_hip.h"))


def header_prototypes(path=HEADER_PATH):
    """{function: [ctypes type per parameter]} parsed from the declarations of include/xmap_hip.h (the single source of
    the C ABI): a pointer of any kind -> c_void_p, int64_t -> c_int64, int / int32_t -> c_int32, float / double."""
    import re
    with open(path) as f:
        text = f.read()
    text = re.sub(r"#\s*ifdef\s+XMAP_CROSSCHECK[^\n]*\n", "\n", text)      # (the guarded prototypes are parsed too: XCHECK_EXPORTS)
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    out = {}
    for m in re.finditer(r"\b(?:int|void|const\s+char\s*\*)\s*(xmap_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        name, args = m.group(1), " ".join(m.group(2).split())
        types = []
        for a in ([] if args in ("", "void") else args.split(",")):
            if "*" in a:
                types.append(C.c_void_p)
            elif "int64_t" in a:
                types.append(C.c_int64)
            elif "double" in a:
                types.append(C.c_double)
            elif "float" in a:
                types.append(C.c_float)
            else:
                types.append(C.c_int32)
        out[name] = types
    return out


def header_constants(prefixes=("XMAP_PAIRS_", "XMAP_LAYOUT_"), path=HEADER_PATH):
    """{name without XMAP_: value} of the header's plain integer #defines with one of the prefixes"""
    import re
    with open(path) as f:
        text = f.read()
    return {n[len("XMAP_"):]: int(v) for n, v in re.findall(r"^#define\s+(XMAP_\w+)\s+(-?\d+)\b", text, flags=re.M)
            if n.startswith(tuple(prefixes))}


def header_structs(path=HEADER_PATH):
    """{struct name: [(member, ctypes type)] in order} of the header's `typedef struct xmap_* { ... }`: a pointer of any
    kind -> c_void_p, int32_t -> c_int32, int64_t -> c_int64 (tests/test_cpu_host.py holds the Structure classes to it)"""
    import re
    with open(path) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    out = {}
    for name, body in re.findall(r"typedef\s+struct\s+(xmap_\w+)\s*\{(.*?)\}\s*\1\s*;", text, flags=re.S):
        out[name] = fields = []
        for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
            kind = C.c_int64 if "int64_t" in decl else C.c_int32 if "int32_t" in decl else None
            for m in decl.split(","):       # (`int32_t n_items, top_k;`: every declarator carries its own `*`)
                fields.append((re.search(r"(\w+)\s*$", m).group(1), C.c_void_p if "*" in m else kind))
    return out


# `shelf_by` by name, from the header's constants (XMAP_SHELF_BY_*)
SHELF_BY = {k[len("SHELF_BY_"):].lower(): v for k, v in header_constants(("XMAP_SHELF_BY_",)).items()}
assert SHELF_BY == {"best": SHELF_BY_BEST, "mean": SHELF_BY_MEAN, "label": SHELF_BY_LABEL}
# `mode` of the quota calls by name, and their limits, from the header's constants (XMAP_QUOTA_*)
_QUOTA = header_constants(("XMAP_QUOTA_",))
QUOTA_MODE = {k[len("QUOTA_"):].lower(): v for k, v in _QUOTA.items() if not k.startswith("QUOTA_MAX_")}
assert QUOTA_MODE == {"cap": QUOTA_CAP, "share": QUOTA_SHARE}
assert (_QUOTA["QUOTA_MAX_POOL"], _QUOTA["QUOTA_MAX_RECORDS"]) == (QUOTA_MAX_POOL, QUOTA_MAX_RECORDS)

assert header_constants(("XMAP_ALLOT_",)) == {"ALLOT_MAX_POOL": ALLOT_MAX_POOL}

# argtypes of every export: a mis-ordered or mis-typed argument raises in ctypes instead of corrupting device memory
PROTOTYPES = header_prototypes()


def _bind(L, names):
    for _n in names:
        _f = getattr(L, _n)
        _f.argtypes = PROTOTYPES[_n]
        if _n in ("xmap_ctx_destroy", "xmap_feed_free"):
            _f.restype = None
        elif _n != "xmap_last_error":
            _f.restype = C.c_int


_bind(lib, [n for n in PROTOTYPES if n not in XCHECK_EXPORTS])
_xlib = None


def xlib():
    """libxmap_hip_xcheck.so: every product entry point + the test formulations.  Loaded on first use (tests, tuning tools:
    Engine.item_sim(algo="rows"), extend(algo="mid"), XMAP_MID_TABLE=1); the pipelines never call it."""
    global _xlib
    if _xlib is None:
        if not os.path.exists(XLIB_PATH):
            raise ImportError("libxmap_hip_xcheck.so not built (%s): make -C x-map_amd/csrc" % XLIB_PATH)
        L = C.CDLL(XLIB_PATH)
        L.xmap_last_error.restype = C.c_char_p
        _bind(L, list(PROTOTYPES))
        _xlib = L
    return _xlib


def check(rc):
    if rc != 0:
        raise XmapError(rc, (lib.xmap_last_error() or b"").decode())


def xcheck(rc):
    if rc != 0:
        raise XmapError(rc, (xlib().xmap_last_error() or b"").decode())


def vp(t):
    """device pointer of a torch tensor (or None)"""
    if t is None:
        return C.c_void_p(0)
    return C.c_void_p(t.data_ptr())


def rec_filter(allow=None, ex_ptr=None, ex_id=None, min_score=None):
    """an xmap_rec_filter over torch tensors (device, for the fine-grained calls) or None; min_score None = no floor.  The
    caller keeps the tensors alive for the call."""
    return RecFilter(None if allow is None else allow.data_ptr(), None if ex_ptr is None else ex_ptr.data_ptr(),
                     None if ex_id is None else ex_id.data_ptr(), float("-inf") if min_score is None else float(min_score))


def i64(v):
    return C.c_int64(int(v))


def i32(v):
    return C.c_int32(int(v))
