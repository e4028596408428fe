"""Geodesic restated twice (include/lbmdem_hip.h, "Geodesic"): for every passable fluid node the cost of the shortest path of
adjacent passable nodes from an inlet region, 5 an axis step and 7 a diagonal one, the same from an outlet region, the corridor
between them, the profile over the depth behind the inlet and the ten counts. restate() relaxes the whole plane by Jacobi sweeps
in numpy until nothing changes; brute_force() is a heap Dijkstra node by node over the grid. files_bytes() spells the files out
as the header states them."""
import heapq

import numpy as np

import clearance_util as cz
from drainage_util import SIDE_B, SIDE_L, SIDE_R, SIDE_T, region

GEODESIC_COUNTERS = ("fluid_nodes", "passable_nodes", "inlet_nodes", "reached_nodes", "dist_max", "outlet_nodes", "outlet_reached",
                     "shortest", "shortest_node", "path_nodes")
DATA_HEADER = ("# t fluid_nodes passable_nodes inlet_nodes reached_nodes dist_max outlet_nodes outlet_reached shortest shortest_node "
               "path_nodes\n")
LEVEL_DTYPE = np.dtype([("nodes", np.int64), ("reached", np.int64), ("sum", np.int64), ("dmin", np.int32), ("dmax", np.int32)])
AXIS, DIAGONAL = 5, 7
INF = np.iinfo(np.int64).max // 4
STEPS4 = ((-1, 0, AXIS), (1, 0, AXIS), (0, -1, AXIS), (0, 1, AXIS))
STEPS8 = STEPS4 + ((-1, -1, DIAGONAL), (-1, 1, DIAGONAL), (1, -1, DIAGONAL), (1, 1, DIAGONAL))


def passable(M, n, min_d2):
    """-> (fluid, passable), bool [lx][ly]; the clearance is only looked at when it can matter"""
    fluid = np.asarray(M) == -1
    if min_d2 <= 1:
        return fluid, fluid.copy()
    return fluid, fluid & (cz.restate(np.asarray(M, dtype=np.int32), n)["d2"] >= min_d2)


def depth(lx, ly, frm):
    """the least offset of every node to a side in frm, int64 [lx][ly]"""
    X, Y = np.meshgrid(np.arange(lx), np.arange(ly), indexing="ij")
    parts = [a for bit, a in ((SIDE_B, Y), (SIDE_T, ly - 1 - Y), (SIDE_L, X), (SIDE_R, lx - 1 - X)) if frm & bit]
    return np.minimum.reduce(parts).astype(np.int64)


def sweeps(P, S, conn):
    """Jacobi sweeps over the passable plane P from the seed S -> (int64 plane with INF where nothing arrives, sweeps made)"""
    lx, ly = P.shape
    D = np.full((lx + 2, ly + 2), INF, np.int64)
    inner = D[1:-1, 1:-1]
    inner[P & S] = 0
    count = 0
    while True:
        count += 1
        best = inner.copy()
        for dx, dy, w in (STEPS8 if conn == 8 else STEPS4):
            np.minimum(best, D[1 + dx:lx + 1 + dx, 1 + dy:ly + 1 + dy] + w, out=best)
        best[~P] = INF
        if np.array_equal(best, inner):
            return inner.copy(), count
        inner[...] = best


def dijkstra(P, S, conn):
    lx, ly = P.shape
    D = np.full(lx * ly, INF, np.int64)
    ok = P.reshape(-1)
    heap = [(0, int(p)) for p in np.nonzero((P & S).reshape(-1))[0]]
    for _, p in heap:
        D[p] = 0
    steps = STEPS8 if conn == 8 else STEPS4
    while heap:
        v, p = heapq.heappop(heap)
        if v > D[p]:
            continue
        x, y = divmod(p, ly)
        for dx, dy, w in steps:
            xq, yq = x + dx, y + dy
            if 0 <= xq < lx and 0 <= yq < ly:
                q = xq * ly + yq
                if ok[q] and v + w < D[q]:
                    D[q] = v + w
                    heapq.heappush(heap, (v + w, q))
    return D.reshape(lx, ly)


def finish(fluid, P, dist, back, frm, band, to, rounds):
    """planes with INF -> everything the contract names"""
    lx, ly = P.shape
    S, T = P & region(lx, ly, frm, band), P & region(lx, ly, to, band)
    reached = dist < INF
    dist = np.where(reached, dist, -1)
    back = np.where(back < INF, back, -1) if to else np.full((lx, ly), -1, np.int64)
    out_reached = T & reached
    shortest = int(dist[out_reached].min()) if out_reached.any() else -1
    at = np.nonzero((out_reached & (dist == shortest)).reshape(-1))[0]
    both = (dist >= 0) & (back >= 0) & (shortest >= 0)
    detour = np.where(both, dist + back - shortest, -1)
    dep = depth(lx, ly, frm)
    nd = int(dep.max()) + 1
    prof = np.zeros(nd, LEVEL_DTYPE)
    prof["nodes"] = np.bincount(dep[P], minlength=nd)
    prof["reached"] = np.bincount(dep[reached], minlength=nd)
    prof["sum"] = np.bincount(dep[reached], weights=dist[reached], minlength=nd).astype(np.int64)
    prof["dmin"] = prof["dmax"] = -1
    lo, hi = np.full(nd, INF, np.int64), np.full(nd, -1, np.int64)
    np.minimum.at(lo, dep[reached], dist[reached])
    np.maximum.at(hi, dep[reached], dist[reached])
    some = prof["reached"] > 0
    prof["dmin"][some], prof["dmax"][some] = lo[some], hi[some]
    c = dict(fluid_nodes=int(fluid.sum()), passable_nodes=int(P.sum()), inlet_nodes=int(S.sum()), reached_nodes=int(reached.sum()),
             dist_max=int(dist.max()) if reached.any() else -1, outlet_nodes=int(T.sum()), outlet_reached=int(out_reached.sum()),
             shortest=shortest, shortest_node=int(at[0]) if len(at) else -1, path_nodes=int((detour == 0).sum()))
    return dict(dist=dist.astype(np.int32), back=back.astype(np.int32), detour=detour.astype(np.int32), profile=prof,
                counts={k: c[k] for k in GEODESIC_COUNTERS}, rounds=rounds)


def restate(M, n, frm, band, to=0, conn=8, min_d2=0):
    """-> dict(dist, back, detour, profile, counts, rounds) of the map M [lx][ly]; rounds: the Jacobi sweeps of the forward and
    the backward relaxation here (the device's launches are its own)"""
    M = np.asarray(M, dtype=np.int32)
    lx, ly = M.shape
    fluid, P = passable(M, n, min_d2)
    dist, r0 = sweeps(P, region(lx, ly, frm, band), conn)
    back, r1 = sweeps(P, region(lx, ly, to, band), conn) if to else (None, 0)
    return finish(fluid, P, dist, back if to else dist, frm, band, to, (r0, r1))


def brute_force(M, n, frm, band, to=0, conn=8, min_d2=0):
    """the same by a heap Dijkstra over the grid"""
    M = np.asarray(M, dtype=np.int32)
    lx, ly = M.shape
    fluid, P = passable(M, n, min_d2)
    dist = dijkstra(P, region(lx, ly, frm, band), conn)
    back = dijkstra(P, region(lx, ly, to, band), conn) if to else dist
    return finish(fluid, P, dist, back, frm, band, to, (0, 0))


def same(A, B):
    """every output of two statements equal -> the name of the first that differs, or None"""
    if A["counts"] != B["counts"]:
        return "counts"
    for name in ("dist", "back", "detour", "profile"):
        if A[name].shape != B[name].shape or not np.array_equal(A[name], B[name]):
            return name
    return None


def files_bytes(lx, ly, n, frm, band, to, conn, min_d2, R, t, nfile=0, plane=False):
    """the files of lbmdem_write_geodesic_files as the header spells them out -> {name: bytes}; geodesic.data: the one line"""
    pr = ["# lx %d ly %d n %d from %d band %d to %d conn %d min_d2 %d\n" % (lx, ly, n, frm, band, to, conn, min_d2),
          "# depth nodes reached sum min max tortuosity\n"]
    for k, e in enumerate(R["profile"]):
        tau = 0.0
        if k >= band and e["reached"] > 0:
            tau = float(int(e["sum"])) / float(AXIS * int(e["reached"]) * (k - band + 1))
        pr.append("%d %d %d %d %d %d %.6f\n" % (k, e["nodes"], e["reached"], e["sum"], e["dmin"], e["dmax"], tau))
    line = "%e" % t + "".join(" %d" % R["counts"][k] for k in GEODESIC_COUNTERS) + "\n"
    out = {"geodesic_profile%06d.dat" % nfile: "".join(pr).encode(), "geodesic.data": line.encode()}
    if plane:
        pas = float(np.float32(1.0 / lx))
        data = ("# vtk DataFile Version 2.0\nlbmdem geodesic\nBINARY\nDATASET STRUCTURED_POINTS\n"
                "DIMENSIONS %d %d 1\nORIGIN 0 0 0\nSPACING %.9g %.9g 1\nPOINT_DATA %d\n" % (lx, ly, pas, pas, lx * ly)).encode()
        for name in ("dist", "back", "detour"):
            data += b"SCALARS %s int 1\nLOOKUP_TABLE default\n" % name.encode()
            data += np.ascontiguousarray(R[name].T).astype(">i4").tobytes() + b"\n"
        out["geodesic%06d.vtk" % nfile] = data
    return out


def comb(lx, ly):
    """corridors one node wide, stacked along y at every other y, separated by walls one node wide and joined at alternating
    ends, over the whole lattice: one path of about lx * ly / 2 nodes that crosses every column of tiles once per corridor"""
    M = np.zeros((lx, ly), np.int32)
    M[:, 0:ly:2] = -1
    for y in range(1, ly - 1, 2):
        M[lx - 1 if y % 4 == 1 else 0, y] = -1
    return M
