"""The statement of xmap_peer_rows_ls (include/xmap_hip.h, "peers"; csrc/stage_e_peers.hip) in plain Python, on top of
peers_statement.peer_rows_statement: the four shared outputs are that statement's, and the local sensitivity of every returned
entry is taken here in the device's operation order -- one rounded fp64 operation per step, no fused multiply-add, the largest
distance chosen as a bit pattern with a NaN above everything (tri.h: ls_key).  Every layer must reproduce it bit for bit."""
import struct

import numpy as np

import peers_statement as ps
from peers_statement import _sqrt, dd_sum

NAN_KEY = 0x7ff8000000000000


def ls_key(d):
    """a distance as an integer that orders like the number; NaN above every number"""
    return NAN_KEY if d != d else struct.unpack("<Q", struct.pack("<d", d))[0]


def _weighted(c, n, cap):
    return 1.0 * c * float(min(n, cap)) / float(cap)


def entry_ls(records, nx, ny, sim, cap):
    """records: [(a_t, b_t)*] in record order -- the x of the query's row and of the holder's row -> ls of the entry.  Python
    floats are fp64 and +, -, *, / round once (a product that overflows is an infinity, no divisor here is zero), so every line
    is one operation of the device"""
    n = len(records)
    inner = dd_sum([a * b for a, b in records])
    nx2, ny2 = nx * nx, ny * ny
    best = 0
    for a, b in records:
        rest = inner - a * b
        m1 = _sqrt((nx2 - a * a) * ny2)
        m2 = _sqrt(nx2 * (ny2 - b * b))
        for m in (m1, m2):
            c = 1.0 * rest / m if m != 0.0 else 0.0                     # NaN != 0: divides
            d = abs(_weighted(c, n - 1, cap) - sim)
            best = max(best, ls_key(d))
    return struct.unpack("<d", struct.pack("<Q", best))[0]


def peer_rows_ls_statement(P, Q, query_user, n_top, cap=1, min_common=1, flags=0, centre=None, allow=None, exclude=None,
                           min_score=None, index=None):
    """-> (cnt, user, sim, common, ls [Q][n_top] (0.0 behind the count), stats): the arguments of peer_rows_statement"""
    X = index or ps.peer_index_statement(P, centre)
    cnt, user, sim, common, stats = ps.peer_rows_statement(P, Q, query_user, n_top, cap, min_common, flags, centre, allow, exclude,
                                                           min_score, X)
    hd_ptr, hd_user, hd_x, nrm = X["hd_ptr"].tolist(), X["hd_user"].tolist(), X["hd_x"].tolist(), X["nrm"].tolist()
    qx, qvalid = ps._x(Q, centre)
    qn = ps._norms(Q, qx, qvalid).tolist()
    qx, qvalid, qptr, qitem = qx.tolist(), qvalid.tolist(), Q.ptr.tolist(), Q.item.tolist()
    ls = np.zeros((len(query_user), n_top))
    for q, a in enumerate(int(u) for u in query_user):
        if cnt[q] == 0:
            continue
        wanted = {int(v): [] for v in user[q, :cnt[q]]}
        for p in range(qptr[a], qptr[a + 1]):                       # the records of the returned users, in record order
            if not qvalid[p]:
                continue
            for h in range(hd_ptr[qitem[p]], hd_ptr[qitem[p] + 1]):
                if hd_user[h] in wanted:
                    wanted[hd_user[h]].append((qx[p], hd_x[h]))
        for j in range(cnt[q]):
            v = int(user[q, j])
            assert len(wanted[v]) == common[q, j]
            ls[q, j] = entry_ls(wanted[v], qn[a], nrm[v], float(sim[q, j]), cap)
    return cnt, user, sim, common, ls, stats


def all_pairs_statement(P, cap):
    """every directed pair of the uncentred profiles P: {(u1, u2): (sim, ls)}, the user itself left out -- the rows of the
    cosine_user similarity in index space"""
    n_top = max(P.n_users, 1)
    cnt, user, sim, _, ls, _ = peer_rows_ls_statement(P, P, np.arange(P.n_users, dtype=np.int32), n_top, cap, 1, ps.SAME)
    return {(q, int(user[q, j])): (float(sim[q, j]), float(ls[q, j])) for q in range(P.n_users) for j in range(cnt[q])}
