"""Drainage restated twice (include/lbmdem_hip.h, "Drainage"): for every fluid node the largest d2 that a path of adjacent fluid
nodes from an inlet side can keep all the way -- the widest path over the clearance analysis' exact squared distance.
restate() works on the pore network, as the device does: the seed and the relaxation over network_util's level-0 link table to
the fixed point, then the plane, pass, the histogram and the ten counts. brute_force() does not use the network at all: a max-heap
widest path node by node over the grid. files_bytes() spells the files out as the header states them."""
import heapq

import numpy as np

import clearance_util as cz
import network_util as nu

SIDE_B, SIDE_T, SIDE_L, SIDE_R = 1, 2, 4, 8
DRAINAGE_COUNTERS = ("fluid_nodes", "inlet_nodes", "reached_nodes", "reached_bodies", "access_max", "shielded_nodes", "outlet_nodes",
                     "critical", "critical_node", "front_links")
NODE_COUNTERS = ("fluid_nodes", "inlet_nodes", "reached_nodes", "access_max", "shielded_nodes", "outlet_nodes", "critical",
                 "critical_node")          # what brute_force() has without a network
DATA_HEADER = ("# t fluid_nodes inlet_nodes reached_nodes reached_bodies access_max shielded_nodes outlet_nodes critical "
               "critical_node front_links\n")


def region(lx, ly, mask, band):
    """the nodes of a side mask's region, bool [lx][ly]"""
    X, Y = np.meshgrid(np.arange(lx), np.arange(ly), indexing="ij")
    out = np.zeros((lx, ly), bool)
    if mask & SIDE_B:
        out |= Y < band
    if mask & SIDE_T:
        out |= Y >= ly - band
    if mask & SIDE_L:
        out |= X < band
    if mask & SIDE_R:
        out |= X >= lx - band
    return out


def node_counts(d2, access, frm, band, to):
    """the counts that need no network, and the histogram"""
    lx, ly = d2.shape
    fluid = d2 > 0
    S, T = fluid & region(lx, ly, frm, band), fluid & region(lx, ly, to, band)
    critical = int(access[T].max()) if T.any() else 0
    at = np.nonzero((T & (access == critical) & (access > 0)).reshape(-1))[0]
    kmax = int(cz.isqrt(int(d2.max())))
    hist = np.bincount(cz.isqrt(access[fluid]), minlength=kmax + 1).astype(np.int64)
    c = dict(fluid_nodes=int(fluid.sum()), inlet_nodes=int(S.sum()), reached_nodes=int((access > 0).sum()),
             access_max=int(access.max()), shielded_nodes=int(((access > 0) & (access < d2)).sum()), outlet_nodes=int(T.sum()),
             critical=critical if to else -1, critical_node=int(at[0]) if len(at) else -1)
    return c, hist


def restate(M, n, frm, band, to, N=None):
    """-> dict(access, A, passes, hist, counts, rounds, network) of the map M [lx][ly]; N: network_util.restate(M, n, -1) if the
    caller has it. rounds: the Jacobi sweeps the relaxation took here (the device's launches are its own)"""
    M = np.asarray(M, dtype=np.int32)
    lx, ly = M.shape
    N = nu.restate(M, n, -1) if N is None else N
    d2, body, links = N["d2"].astype(np.int64), N["body"], N["links0"]
    fluid = M == -1
    B = len(N["bodies"])
    S = fluid & region(lx, ly, frm, band)
    A = np.zeros(B, np.int64)
    np.maximum.at(A, body[S], d2[S])
    lo, hi, sd = links["lo"].astype(np.int64), links["hi"].astype(np.int64), links["saddle"].astype(np.int64)
    rounds = 0
    while len(links):
        rounds += 1
        nxt = A.copy()
        np.maximum.at(nxt, lo, np.minimum(A[hi], sd))
        np.maximum.at(nxt, hi, np.minimum(A[lo], sd))
        if np.array_equal(nxt, A):
            break
        A = nxt
    access = np.where(fluid, np.minimum(d2, A[np.where(fluid, body, 0)] if B else 0), 0).astype(np.int32)
    passes = np.minimum(np.minimum(A[lo], A[hi]), sd).astype(np.int32)
    c, hist = node_counts(N["d2"], access, frm, band, to)
    crit = c["critical"]
    front = int(((sd == crit) & (np.maximum(A[lo], A[hi]) > crit) & (np.minimum(A[lo], A[hi]) == crit)).sum()) if crit > 0 else 0
    c.update(reached_bodies=int((A > 0).sum()), front_links=front)
    return dict(access=access, A=A.astype(np.int32), passes=passes, hist=hist, counts={k: c[k] for k in DRAINAGE_COUNTERS},
                rounds=rounds, network=N)


def brute_force(M, n, frm, band, to):
    """-> dict(access, hist, counts of NODE_COUNTERS): a max-heap widest path over the grid and clearance_util's d2"""
    M = np.asarray(M, dtype=np.int32)
    lx, ly = M.shape
    d2 = cz.restate(M, n)["d2"]
    D = d2.reshape(-1)
    S = ((M == -1) & region(lx, ly, frm, band)).reshape(-1)
    access = np.zeros(lx * ly, np.int64)
    heap = [(-int(D[p]), int(p)) for p in np.nonzero(S)[0]]
    for v, p in heap:
        access[p] = -v
    heapq.heapify(heap)
    while heap:
        v, p = heapq.heappop(heap)
        if -v < access[p]:
            continue
        x, y = divmod(p, ly)
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                xq, yq = x + dx, y + dy
                if (dx or dy) and 0 <= xq < lx and 0 <= yq < ly:
                    q = xq * ly + yq
                    w = min(-v, int(D[q]))
                    if w > access[q]:          # (off the fluid D is 0: never)
                        access[q] = w
                        heapq.heappush(heap, (-w, q))
    access = access.reshape(lx, ly).astype(np.int32)
    c, hist = node_counts(d2, access, frm, band, to)
    return dict(access=access, hist=hist, counts=c)


def same(A, B):
    """every output of the device and the restatement equal -> the name of the first that differs, or None"""
    if A["counts"] != B["counts"]:
        return "counts"
    for name in ("access", "A", "passes", "hist"):
        if A[name].shape != B[name].shape or not np.array_equal(A[name], B[name]):
            return name
    return None


def files_bytes(lx, ly, n, frm, band, to, R, clearance_hist, t, nfile=0, plane=False):
    """the files of lbmdem_write_drainage_files as the header spells them out -> {name: bytes}; drainage.data: the one line"""
    first = "# lx %d ly %d n %d from %d band %d to %d\n" % (lx, ly, n, frm, band, to)
    hist = R["hist"]
    cu = [first, "# k access_nodes clearance_nodes invaded\n"]
    for k in range(len(hist)):
        cu.append("%d %d %d %d\n" % (k, hist[k], clearance_hist[k], int(hist[max(k, 1):].sum())))
    bo = [first, "# body node d2 A\n"]
    for i, e in enumerate(R["network"]["bodies"]):
        bo.append("%d %d %d %d\n" % (i, e["node"], e["d2"], R["A"][i]))
    line = "%e" % t + "".join(" %d" % R["counts"][k] for k in DRAINAGE_COUNTERS) + "\n"
    out = {"drainage_curve%06d.dat" % nfile: "".join(cu).encode(), "drainage_bodies%06d.dat" % nfile: "".join(bo).encode(),
           "drainage.data": line.encode()}
    if plane:
        pas = float(np.float32(1.0 / lx))
        data = ("# vtk DataFile Version 2.0\nlbmdem drainage\nBINARY\nDATASET STRUCTURED_POINTS\n"
                "DIMENSIONS %d %d 1\nORIGIN 0 0 0\nSPACING %.9g %.9g 1\nPOINT_DATA %d\n" % (lx, ly, pas, pas, lx * ly)).encode()
        data += b"SCALARS access int 1\nLOOKUP_TABLE default\n"
        data += np.ascontiguousarray(R["access"].T).astype(">i4").tobytes() + b"\n"
        out["drainage%06d.vtk" % nfile] = data
    return out


# ---- the maps: solid is grain 0, (lx, ly) at least 40 x 40 unless stated ----

def random_discs(lx, ly, n, seed):
    rng = np.random.default_rng(seed)
    count = max(3, lx * ly // 260)
    rmax = max(2.0, min(lx, ly) / 9.0)
    return cz.disc_map(lx, ly, [(rng.uniform(0, lx), rng.uniform(0, ly), rng.uniform(1.0, rmax), k % n) for k in range(count)])


def two_pores(lx, ly):
    """two pores apart: one at low y, one at high y"""
    M = np.zeros((lx, ly), np.int32)
    M[1:lx - 1, 0:ly // 2 - 2] = -1
    M[1:lx - 1, ly // 2 + 2:ly] = -1
    return M


def chamber_behind_neck(lx, ly):
    """a reservoir 5 deep at low y, a neck one node wide, a chamber 17 wide behind it"""
    M = np.zeros((lx, ly), np.int32)
    cx = lx // 2
    M[:, 0:5] = -1
    M[cx, 5:11] = -1
    M[cx - 8:cx + 9, 11:29] = -1
    return M


def diagonal_passage(lx, ly):
    """two halves joined only by a diagonal step between two solid corners"""
    M = np.full((lx, ly), -1, np.int32)
    h = ly // 2
    M[:, h:h + 2] = 0
    M[lx // 3, h] = -1
    M[lx // 3 + 1, h + 1] = -1
    return M


def two_routes(lx, ly):
    """a reservoir at low y, a chamber at high y, two channels 3 wide between them"""
    M = np.zeros((lx, ly), np.int32)
    M[:, 0:6] = -1
    M[:, ly - 8:ly] = -1
    M[6:9, 6:ly - 8] = -1
    M[lx - 11:lx - 8, 6:ly - 8] = -1
    return M


def serpentine(lx=70, ly=200):
    """corridors 5 wide along x, stacked along y and joined at alternating ends, with a solid node on the centre line every fourth
    x, and a shaft from the last corridor to the top: some hundreds of bodies in series, more level-0 links than the 256 one
    workgroup of the device's relaxation holds"""
    M = np.zeros((lx, ly), np.int32)
    rows = (ly - 2) // 10
    for k in range(rows):
        y0 = 10 * k + 2
        M[2:lx - 2, y0:y0 + 5] = -1
        M[6:lx - 6:4, y0 + 2] = 0
        x0 = lx - 7 if k % 2 == 0 else 2
        M[x0:x0 + 5, y0 + 5:y0 + 10 if k + 1 < rows else ly] = -1
    return M
