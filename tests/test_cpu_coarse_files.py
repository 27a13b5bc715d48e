"""The coarse ABI (xmap_ctx_*) lives in several files of csrc/ -- ctx.h, api.hip, api_tail.hip, api_lists.hip -- and the Makefile
lists what it builds by hand.  A file that is named there and does not exist, a coarse file that is not named there, or an entry
that lost its extern "C" when it moved, shows here without a device: every xmap_ctx_* function the header declares is exported
by both libraries."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "x-map_amd", "csrc")


def _makefile_list(name):
    mk = open(os.path.join(CSRC, "Makefile")).read()
    m = re.search(r"^%s :=(.*)$" % name, mk, flags=re.M)
    assert m, "the Makefile has no %s" % name
    return m.group(1).split()


def test_every_file_the_makefile_names_exists():
    srcs, hdrs = _makefile_list("SRCS"), _makefile_list("HDRS")
    assert len(srcs) > 30 and len(hdrs) > 10
    for f in srcs + hdrs:
        assert os.path.exists(os.path.join(CSRC, f)), "%s is named in the Makefile and does not exist" % f


def test_the_makefile_builds_the_coarse_abi_files():
    srcs, hdrs = _makefile_list("SRCS"), _makefile_list("HDRS")
    for f in ("api.hip", "api_tail.hip", "api_lists.hip"):
        assert f in srcs, f
    assert "ctx.h" in hdrs


def test_every_declared_coarse_entry_is_exported_by_both_libraries():
    hdr = open(os.path.join(ROOT, "include", "xmap_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    names = sorted(set(re.findall(r"\b(xmap_ctx_\w+)\s*\(", hdr)))
    assert len(names) >= 50 and "xmap_ctx_create" in names and "xmap_ctx_recommend_hybrid" in names and "xmap_ctx_evaluate_topn" in names
    from xmap.engine import hipabi
    X = hipabi.xlib()
    for n in names:
        assert hasattr(hipabi.lib, n), "%s is declared and libxmap_hip.so does not export it" % n
        assert hasattr(X, n), "%s is declared and libxmap_hip_xcheck.so does not export it" % n
