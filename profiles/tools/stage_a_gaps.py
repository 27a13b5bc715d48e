"""stage-A span, idle gaps and dispatch count per step from a rocprofv3 kernel trace csv"""
import csv
import glob
import sys

d = sys.argv[1]
files = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)
assert files, "no kernel trace under " + d
rows = []
for f in files:
    with open(f) as fh:
        for r in csv.DictReader(fh):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
rows.sort()
print("kernels in trace:", len(rows))
COUNT = ("k_count3", "k_cbs", "k_cb_count")
# the last kernel of the mirror: k_mir_tiles, or k_mir_large in a trace from before level B finished the large keys
LAST = "k_mir_large" if any("k_mir_large" in r[2] for r in rows) else "k_mir_tiles"
ends = [x for x, r in enumerate(rows) if LAST in r[2]]
sorts = [x for x, r in enumerate(rows) if "k_sort_profiles3" in r[2]]
print(LAST + ":", len(ends), "k_sort_profiles3:", len(sorts))
res = []
for s in sorts:
    e = next((x for x in ends if x > s), None)
    if e is None:
        continue
    # the rater count: walk back from the profile sort to the first count kernel of this pass
    prev_end = max([x for x in ends if x < s], default=-1)
    first = None
    for x in range(prev_end + 1, s):
        if any(c in rows[x][2] for c in COUNT):
            first = x
            break
    if first is None:
        continue
    # a fill in front of the count belongs to it
    while first - 1 > prev_end and "fill" in rows[first - 1][2].lower() and rows[first][0] - rows[first - 1][1] < 50000:
        first -= 1
    span = rows[e][1] - rows[first][0]
    busy_end = rows[first][1]
    idle = 0
    gaps = []
    for x in range(first + 1, e + 1):
        if rows[x][0] > busy_end:
            idle += rows[x][0] - busy_end
            gaps.append((rows[x][0] - busy_end, rows[x - 1][2][:40], rows[x][2][:40]))
        busy_end = max(busy_end, rows[x][1])
    res.append((span, idle, e - first + 1, gaps, first, e))
for k, (span, idle, n, gaps, first, e) in enumerate(res):
    print("step %d: span %.3f ms  idle %.3f ms  dispatches %d" % (k, span / 1e6, idle / 1e6, n))
if res:
    span, idle, n, gaps, first, e = res[-1]
    gaps.sort(reverse=True)
    print("largest gaps of the last step (us, after, before):")
    for g in gaps[:12]:
        print("  %8.1f  %s -> %s" % (g[0] / 1e3, g[1], g[2]))
    if len(sys.argv) > 2:
        print("sequence of the last step:")
        for x in range(first, e + 1):
            print("  %9.1f %8.1f %s" % ((rows[x][0] - rows[first][0]) / 1e3, (rows[x][1] - rows[x][0]) / 1e3, rows[x][2][:70]))
