"""The network pressures restated in numpy (include/lbmdem_hip.h, "Network pressures"): the pore network of network_util.restate as
a resistor network between the regions on an inlet side (p = 1) and those on an outlet side (p = 0), solved by the
Jacobi-preconditioned conjugate gradient whose every operation the header spells out. Every sum is formed in the header's order --
a row as a chain over its links in ascending index (here: the rows padded to the largest degree and added column by column), a dot
product as the tree of rule 4 (a reshape and eight slice additions per level) -- so the device has to reproduce every double on
the bits. numpy multiplies and adds element by element and rounds each result: there is no fused multiply-add to avoid."""
import numpy as np

import drainage_util as du
import network_util as nz

NETSOLVE_REGION_DTYPE = np.dtype([("p", np.float64), ("net", np.float64), ("flags", np.int32), ("degree", np.int32)])
NETSOLVE_LINK_DTYPE = np.dtype([("g", np.float64), ("q", np.float64)])
NETSOLVE_COUNTERS = ("regions", "links", "inlet_regions", "outlet_regions", "shorted_regions", "free_regions", "iterations", "status",
                     "flowing_links", "strongest_link")
NETSOLVE_SUMS = ("Q_in", "Q_out", "rz0", "rz")
DATA_HEADER = ("# t regions links inlet_regions outlet_regions shorted_regions free_regions iterations status flowing_links "
               "strongest_link Q_in Q_out rz0 rz\n")
AUTO_CAP = 100000


def dot(u, v):
    """rule 4"""
    t = u * v
    if len(t) == 0:
        return 0.0
    while True:
        pad = -len(t) % 256
        t = np.concatenate([t, np.zeros(pad)]).reshape(-1, 256)
        s = 128
        while s >= 1:
            t = t[:, :s] + t[:, s:2 * s]
            s //= 2
        t = t[:, 0]
        if len(t) == 1:
            return float(t[0])


def regions_of(N, level):
    """per region of the level: the plane of region indices (-1 off the fluid), the (root) body numbers, the peak nodes"""
    if level == 0:
        return N["body"].astype(np.int64), np.arange(len(N["bodies"]), dtype=np.int64), N["bodies"]["node"].astype(np.int64)
    roots = N["groups"]["body"].astype(np.int64)
    g = N["group"].astype(np.int64)
    return np.where(g >= 0, np.searchsorted(roots, np.maximum(g, 0)), -1), roots, N["groups"]["node"].astype(np.int64)


def conductance(table, lo, hi, node, ly):
    """rule 2, model 0"""
    w = 2.0 * np.sqrt(table["saddle"].astype(np.float64))
    dx = node[hi] // ly - node[lo] // ly
    dy = node[hi] % ly - node[lo] % ly
    length = np.sqrt((dx * dx + dy * dy).astype(np.float64))
    return ((w * w) * w) / (12.0 * length)


class Rows:
    """rule 3: per region its links in ascending link index, padded to the largest degree; chain() adds column by column"""

    def __init__(self, R, lo, hi, g):
        L = len(lo)
        own = np.concatenate([lo, hi])
        other = np.concatenate([hi, lo])
        link = np.concatenate([np.arange(L), np.arange(L)])
        order = np.lexsort((link, own))
        own, other, link = own[order], other[order], link[order]
        self.degree = np.bincount(own, minlength=R).astype(np.int64) if R else np.zeros(0, np.int64)
        start = np.concatenate([[0], np.cumsum(self.degree)])[:-1] if R else np.zeros(0, np.int64)
        self.width = int(self.degree.max()) if R and L else 0
        self.partner = np.zeros((R, self.width), np.int64)
        self.g = np.zeros((R, self.width))
        self.there = np.zeros((R, self.width), bool)
        col = np.arange(len(own)) - start[own] if len(own) else np.zeros(0, np.int64)
        self.partner[own, col] = other
        self.g[own, col] = g[link]
        self.there[own, col] = True
        assert not len(own) or (np.diff(self.partner, axis=1)[self.there[:, 1:]] > 0).all()   # ascending partner number

    def chain(self, terms, where=None):
        """per region the chain from +0.0 over its row of terms [R][width], only the entries `where` (default: all that are there)"""
        take = self.there if where is None else self.there & where
        s = np.zeros(len(self.degree))
        for c in range(self.width):
            s = np.where(take[:, c], s + terms[:, c], s)
        return s


def restate(M, n, frm, band, to, merge, level, model=0, g_user=None, rtol=1e-8, max_iter=0, N=None):
    """-> dict(regions, links, counts, sums, table, region_body, and the solver's own: A's pieces for the host tests) of the map M
    [lx][ly]; N: network_util.restate(M, n, merge) where the caller has it"""
    M = np.asarray(M, dtype=np.int32)
    lx, ly = M.shape
    if N is None:
        N = nz.restate(M, n, merge)
    reg, bodyno, node = regions_of(N, level)
    table = N["links1" if level else "links0"]
    R, L = len(bodyno), len(table)
    place = np.full(int(bodyno.max()) + 1 if R else 1, -1, np.int64)
    place[bodyno] = np.arange(R)
    lo, hi = place[table["lo"]], place[table["hi"]]
    fluid = M == -1
    # 1. the fixed regions
    flags = np.zeros(R, np.int32)
    S, T = fluid & du.region(lx, ly, frm, band), fluid & du.region(lx, ly, to, band)
    inlet, outlet = np.zeros(R, bool), np.zeros(R, bool)
    inlet[reg[S]] = True
    outlet[reg[T]] = True
    flags[inlet] = 1
    flags[inlet & outlet] = 5
    flags[~inlet & outlet] = 2
    free = flags == 0
    # 2. the conductances
    g = conductance(table, lo, hi, node, ly) if model == 0 else np.asarray(g_user, dtype=np.float64).copy()
    assert len(g) == L and (g > 0).all() and np.isfinite(g).all()
    # 3. the rows
    rows = Rows(R, lo, hi, g)
    diag = rows.chain(rows.g)
    b = np.where(free, rows.chain(rows.g, inlet[rows.partner]), 0.0)

    def apply(v):
        s = rows.chain(rows.g * v[rows.partner])
        return np.where(free, diag * v - s, 0.0)

    def precondition(r):
        ok = free & (diag > 0)
        return np.where(ok, r / np.where(ok, diag, 1.0), 0.0)
    # 5. the iteration
    limit = max_iter if max_iter > 0 else min(int(free.sum()), AUTO_CAP)
    x = np.zeros(R)
    r = b.copy()
    z = precondition(r)
    d = z.copy()
    rz0 = rz = last = dot(r, z)
    tol2 = rtol * rtol
    status, k = 0, 0
    if rz0 != 0:
        while True:
            k += 1
            q = apply(d)
            dq = dot(d, q)
            if not np.isfinite(dq) or dq <= 0:
                status, k = 2, k - 1
                break
            alpha = rz / dq
            x = x + alpha * d
            r = r - alpha * q
            z = precondition(r)
            rzn = last = dot(r, z)
            if rzn <= tol2 * rz0:
                break
            if k == limit:
                status = 1
                break
            beta = rzn / rz
            d = z + beta * d
            rz = rzn
    # 6. the outputs
    p = np.where(flags & 1, 1.0, np.where(flags & 2, 0.0, x))
    regions = np.zeros(R, NETSOLVE_REGION_DTYPE)
    regions["p"] = p
    regions["net"] = rows.chain(rows.g * (p[rows.partner] - p[:, None])) if R else 0.0
    regions["flags"], regions["degree"] = flags, rows.degree
    links = np.zeros(L, NETSOLVE_LINK_DTYPE)
    links["g"] = g
    links["q"] = g * (p[lo] - p[hi])
    is_in, is_out = (flags & 1) != 0, flags == 2
    sums = dict(Q_in=dot(np.where(is_in, -regions["net"], 0.0), np.ones(R)), Q_out=dot(np.where(is_out, regions["net"], 0.0), np.ones(R)),
                rz0=rz0, rz=last)
    counts = dict(zip(NETSOLVE_COUNTERS, (
        R, L, int(is_in.sum()), int(is_out.sum()), int((flags == 5).sum()), int(free.sum()), k, status, int((links["q"] != 0).sum()),
        int(np.argmax(np.abs(links["q"]).view(np.int64))) if L else -1)))
    return dict(regions=regions, links=links, counts=counts, sums=sums, table=table, region_body=bodyno.astype(np.int32),
                lo=lo, hi=hi, g=g, free=free, inlet=is_in, b=b, x=x, limit=limit)


def same(A, B):
    """every output of the device and the restatement (or of two restatements) equal, doubles on the bits -> the name of the
    first that differs, or None"""
    if A["counts"] != B["counts"]:
        return "counts"
    for k in NETSOLVE_SUMS:
        if np.float64(A["sums"][k]).view(np.int64) != np.float64(B["sums"][k]).view(np.int64):
            return "sums." + k
    for name, dt in (("regions", NETSOLVE_REGION_DTYPE), ("links", NETSOLVE_LINK_DTYPE)):
        if len(A[name]) != len(B[name]):
            return name
        for f in dt.names:
            a, b = np.ascontiguousarray(A[name][f]), np.ascontiguousarray(B[name][f])
            if a.dtype == np.float64:
                a, b = a.view(np.int64), b.view(np.int64)
            if not np.array_equal(a, b):
                return name + "." + f
    return None


def anchored(W):
    """per region: its connected component of the network holds a fixed region (the free ones among them make a regular matrix)"""
    reach = ~W["free"]
    while True:
        nxt = reach.copy()
        np.logical_or.at(nxt, W["lo"], reach[W["hi"]])
        np.logical_or.at(nxt, W["hi"], reach[W["lo"]])
        if np.array_equal(nxt, reach):
            return reach
        reach = nxt


def dense(W):
    """-> (A, rhs, f): the matrix and the right-hand side of the free regions f that are anchored, for numpy.linalg: A[i][i] the
    sum of g over i's links, A[i][j] = -g between free i and j, rhs[i] the sum of g towards inlets"""
    R = len(W["regions"])
    A = np.zeros((R, R))
    np.add.at(A, (W["lo"], W["hi"]), -W["g"])
    np.add.at(A, (W["hi"], W["lo"]), -W["g"])
    deg = np.zeros(R)
    np.add.at(deg, W["lo"], W["g"])
    np.add.at(deg, W["hi"], W["g"])
    A[np.arange(R), np.arange(R)] = deg
    rhs = np.zeros(R)
    np.add.at(rhs, W["lo"], np.where(W["inlet"][W["hi"]], W["g"], 0.0))
    np.add.at(rhs, W["hi"], np.where(W["inlet"][W["lo"]], W["g"], 0.0))
    f = np.nonzero(W["free"] & anchored(W))[0]
    return A[np.ix_(f, f)], rhs[f], f


def files_bytes(lx, ly, n, merge, level, frm, band, to, W, t, nfile=0):
    """the files of lbmdem_write_netsolve_files as the header spells them out -> {name: bytes}; netsolve.data: the one line"""
    first = "# lx %d ly %d n %d merge %d level %d from %d band %d to %d\n" % (lx, ly, n, merge, level, frm, band, to)
    rg = [first, "# region body flags degree p net\n"]
    for k, e in enumerate(W["regions"]):
        rg.append("%d %d %d %d %.17g %.17g\n" % (k, W["region_body"][k], e["flags"], e["degree"], e["p"], e["net"]))
    li = [first, "# lo hi saddle g q\n"]
    for e, s in zip(W["table"], W["links"]):
        li.append("%d %d %d %.17g %.17g\n" % (e["lo"], e["hi"], e["saddle"], s["g"], s["q"]))
    line = ("%e" % t + "".join(" %d" % W["counts"][k] for k in NETSOLVE_COUNTERS) + "".join(" %.17g" % W["sums"][k] for k in NETSOLVE_SUMS)
            + "\n")
    return {"netsolve_regions%06d.dat" % nfile: "".join(rg).encode(), "netsolve_links%06d.dat" % nfile: "".join(li).encode(),
            "netsolve.data": line.encode()}


# ---- the maps: solid is grain 0 ----

def star(size=75, margin=8):
    """a square chamber of size^2 nodes with a small chamber of 3 x 3 nodes every fourth node along each of its four sides, each
    joined to it by a one-node neck: 4 * ((size - 3) // 4 + 1) links in the row of the one body the chamber is. With band 5 the
    small chambers at low y hold inlet nodes (SIDE_B) and those at high y outlet nodes (SIDE_T); the others are dead ends"""
    n = size + 2 * margin
    M = np.zeros((n, n), np.int32)
    c0, c1 = margin, margin + size
    M[c0:c1, c0:c1] = -1
    for t in range(c0 + 1, c1 - 1, 4):
        M[c0 - 1, t] = M[c1, t] = M[t, c0 - 1] = M[t, c1] = -1
        M[c0 - 4:c0 - 1, t - 1:t + 2] = -1
        M[c1 + 1:c1 + 4, t - 1:t + 2] = -1
        M[t - 1:t + 2, c0 - 4:c0 - 1] = -1
        M[t - 1:t + 2, c1 + 1:c1 + 4] = -1
    return M


def chambers(lx, ly, period=5):
    """small chambers of (period - 2)^2 nodes on a square grid, each joined to the next in x and in y by a one-node neck"""
    M = np.zeros((lx, ly), np.int32)
    w = period - 2
    for ox in range(w):
        for oy in range(w):
            M[1 + ox:lx - period + 1:period, 1 + oy:ly - period + 1:period] = -1
    mid = 1 + w // 2
    for o in (w, w + 1):
        M[1 + o:lx - 2 * period + 1 + o:period, mid:ly - period + 1:period] = -1      # necks along x
        M[mid:lx - period + 1:period, 1 + o:ly - 2 * period + 1 + o:period] = -1      # necks along y
    return M
