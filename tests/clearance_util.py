"""The pore clearance analysis restated in numpy (include/lbmdem_hip.h, "Pore clearance"): the map padded with one ring of wall
nodes, a packed key d2 << 32 | owner minimised along y and then along x, the histogram, the owners' table, the ridge by lexsort,
the ten counts and the files exactly as the header states them -- every result is an integer, so the device has to reproduce every
one of them. And the maps the tests measure: pore_util's, plus the shapes a distance search gets wrong."""
import numpy as np

import pore_util

THROAT_DTYPE = np.dtype([("lo", np.int32), ("hi", np.int32), ("edges", np.int32), ("c_min", np.int32), ("node", np.int32)])
CLEARANCE_COUNTERS = ("fluid_nodes", "d2_max", "d2_max_node", "sum_d2", "ridge_edges", "throats", "grain_throats", "narrowest_c",
                      "ownerless_grains", "kmax")
DATA_HEADER = "# t fluid_nodes d2_max d2_max_node sum_d2 ridge_edges throats grain_throats narrowest_c ownerless_grains kmax\n"
BIG = np.iinfo(np.int64).max


def padded(M, n):
    """the map with one ring of n round it: every position outside the lattice counts as a wall node, and no position further
    out is nearer to a node of the lattice than the ring's"""
    M = np.asarray(M, dtype=np.int64)
    P = np.full((M.shape[0] + 2, M.shape[1] + 2), n, np.int64)
    P[1:-1, 1:-1] = M
    return P


def isqrt(v):
    """floor(sqrt(v)) of non-negative int64, in integers: the float estimate corrected"""
    v = np.asarray(v, dtype=np.int64)
    r = np.floor(np.sqrt(v.astype(np.float64))).astype(np.int64)
    r = np.where(r * r > v, r - 1, r)
    return np.where((r + 1) * (r + 1) <= v, r + 1, r)


def distance_keys(M, n):
    """-> key [lx][ly] int64, d2 << 32 | owner: per node the minimum over all non-fluid positions of the padded map"""
    P = padded(M, n)
    px, py = P.shape
    solid = P >= 0
    Y = np.broadcast_to(np.arange(py, dtype=np.int64), P.shape)
    # along y: the nearest non-fluid position at or below and at or above (columns 0 and py - 1 are wall)
    dn = np.maximum.accumulate(np.where(solid, Y, -1), axis=1)
    up = np.minimum.accumulate(np.where(solid, Y, py)[:, ::-1], axis=1)[:, ::-1]
    rows = np.arange(px)[:, None]
    kd = ((Y - dn) ** 2 << 32) | P[rows, dn]
    ku = ((up - Y) ** 2 << 32) | P[rows, up]
    row = np.minimum(kd, ku)
    # along x: the minimum over x' of (x - x')^2 << 32 added to the row's key; dx beyond the root of the best cannot win
    best = row.copy()
    for dx in range(1, px):
        if dx * dx > int((best >> 32).max()):
            break
        add = np.int64(dx * dx) << 32
        best[dx:] = np.minimum(best[dx:], row[:-dx] + add)
        best[:-dx] = np.minimum(best[:-dx], row[dx:] + add)
    return best[1:-1, 1:-1]


def brute_force(M, n):
    """the same keys by a loop over all pairs of (node, non-fluid position): small maps only"""
    P = padded(M, n)
    sx, sy = np.nonzero(P >= 0)
    so = P[sx, sy]
    lx, ly = np.asarray(M).shape
    key = np.zeros((lx, ly), np.int64)
    for x in range(lx):
        for y in range(ly):
            d = (sx - (x + 1)) ** 2 + (sy - (y + 1)) ** 2
            key[x, y] = ((d << 32) | so).min()
    return key


def restate(M, n):
    """-> dict(d2, owner, hist, owned, d2max, table, counts) of the map M [lx][ly] (-1 fluid, 0 .. n - 1 a grain, n the wall)"""
    M = np.asarray(M, dtype=np.int32)
    lx, ly = M.shape
    key = distance_keys(M, n)
    return from_keys(M, n, key)


def from_keys(M, n, key):
    M = np.asarray(M, dtype=np.int32)
    lx, ly = M.shape
    d2 = (key >> 32).astype(np.int32)
    owner = (key & 0xFFFFFFFF).astype(np.int32)
    fluid = M == -1
    assert ((d2 > 0) == fluid).all() and (owner[~fluid] == M[~fluid]).all()
    d2_max = int(d2.max())
    kmax = int(isqrt(d2_max))
    hist = np.bincount(isqrt(d2[fluid]), minlength=kmax + 1).astype(np.int64)
    owned = np.bincount(owner[fluid], minlength=n + 1).astype(np.int64)
    d2max = np.full(n + 1, -1, np.int64)
    np.maximum.at(d2max, owner[fluid], d2[fluid])
    idx = np.arange(lx * ly, dtype=np.int64).reshape(lx, ly)
    lo, hi, c, p = [], [], [], []
    for a, b in (((slice(None), slice(0, ly - 1)), (slice(None), slice(1, ly))), ((slice(0, lx - 1), slice(None)), (slice(1, lx), slice(None)))):
        m = fluid[a] & fluid[b] & (owner[a] != owner[b])
        lo.append(np.minimum(owner[a], owner[b])[m]); hi.append(np.maximum(owner[a], owner[b])[m])
        c.append(np.maximum(d2[a], d2[b])[m]); p.append(idx[a][m])
    lo, hi, c, p = (np.concatenate(v).astype(np.int64) for v in (lo, hi, c, p))
    order = np.lexsort((p, c, hi, lo))
    lo, hi, c, p = lo[order], hi[order], c[order], p[order]
    head = np.ones(len(lo), bool)
    head[1:] = (lo[1:] != lo[:-1]) | (hi[1:] != hi[:-1])
    first = np.nonzero(head)[0]
    table = np.zeros(len(first), THROAT_DTYPE)
    table["lo"], table["hi"], table["c_min"], table["node"] = lo[first], hi[first], c[first], p[first]
    table["edges"] = np.diff(np.append(first, len(lo)))
    gg = table["hi"] < n
    counts = dict(zip(CLEARANCE_COUNTERS, (int(fluid.sum()), d2_max, int(np.argmax(d2.reshape(-1))), int(d2.astype(np.int64).sum()),
                                           len(lo), len(table), int(gg.sum()), int(table["c_min"][gg].min()) if gg.any() else -1,
                                           int((owned[:n] == 0).sum()), kmax)))
    return dict(d2=d2, owner=owner, hist=hist, owned=owned, d2max=d2max.astype(np.int32), table=table, counts=counts)


def files_bytes(lx, ly, n, R, t, nfile=0, plane=False):
    """the files of lbmdem_write_clearance_files as the header spells them out -> {name: bytes}; clearance.data: the one line"""
    th = ["# lx %d ly %d n %d\n" % (lx, ly, n), "# lo hi edges c_min node\n"]
    for e in R["table"]:
        th.append("%d %d %d %d %d\n" % (e["lo"], e["hi"], e["edges"], e["c_min"], e["node"]))
    hs = ["# k nodes\n"] + ["%d %d\n" % (k, v) for k, v in enumerate(R["hist"])]
    ow = ["# owner owned d2max\n"] + ["%d %d %d\n" % (i, R["owned"][i], R["d2max"][i]) for i in range(n + 1)]
    line = "%e" % t + "".join(" %d" % R["counts"][k] for k in CLEARANCE_COUNTERS) + "\n"
    out = {"throats%06d.dat" % nfile: "".join(th).encode(), "clearance_hist%06d.dat" % nfile: "".join(hs).encode(),
           "clearance_owners%06d.dat" % nfile: "".join(ow).encode(), "clearance.data": line.encode()}
    if plane:
        pas = float(np.float32(1.0 / lx))
        body = ("# vtk DataFile Version 2.0\nlbmdem pore clearance\nBINARY\nDATASET STRUCTURED_POINTS\n"
                "DIMENSIONS %d %d 1\nORIGIN 0 0 0\nSPACING %.9g %.9g 1\nPOINT_DATA %d\n" % (lx, ly, pas, pas, lx * ly)).encode()
        for name in ("d2", "owner"):
            body += ("SCALARS %s int 1\nLOOKUP_TABLE default\n" % name).encode()
            body += np.ascontiguousarray(R[name].T).astype(">i4").tobytes() + b"\n"
        out["clearance%06d.vtk" % nfile] = body
    return out


# ---- the maps ----

def disc_map(lx, ly, discs):
    """discs: (cx, cy, r, owner) -> map with the nodes within r of a centre owned, the rest fluid; later discs overwrite"""
    X, Y = np.meshgrid(np.arange(lx), np.arange(ly), indexing="ij")
    M = np.full((lx, ly), -1, np.int32)
    for cx, cy, r, o in discs:
        M[(X - cx) ** 2 + (Y - cy) ** 2 <= r * r] = o
    return M


def two_discs(lx, ly, n):
    """two pairs of discs along y, one with its nearest solid nodes an even number apart (6), one odd (5)"""
    r = max(2, min(10, (ly - 10) // 4, (lx - 6) // 4))
    out = []
    for k, gap in enumerate((6, 5)):
        cx = (lx // 4) * (1 + 2 * k)
        cy = 1 + r
        out += [(cx, cy, r, (2 * k) % n), (cx, cy + 2 * r + gap, r, (2 * k + 1) % n)]
    return disc_map(lx, ly, out)


def shape_maps(lx, ly, n):
    """name -> map [lx][ly]: every map of pore_util.shape_maps, and the cases of a distance search"""
    out = dict(pore_util.shape_maps(lx, ly, n))
    # five solid nodes, one of them in a corner
    M = np.full((lx, ly), -1, np.int32)
    for k, (x, y) in enumerate(((0, 0), (lx // 2, ly // 3), (lx - 2, ly - 1), (lx // 3, ly - 2), (2 * lx // 3, 1))):
        M[x, y] = k % (n + 1)
    out["sparse_seeds"] = M
    # a single solid column at x = 0
    M = np.full((lx, ly), -1, np.int32)
    M[0, :] = 0
    out["far_wall"] = M
    out["two_discs"] = two_discs(lx, ly, n)
    # solid nodes of different owners placed symmetrically about fluid nodes, along y, along x and along the diagonals: the
    # larger owner comes first in node order every second time, so that only the rule decides
    M = np.full((lx, ly), -1, np.int32)
    hi, lo = min(n - 1, 3), 0
    cx, cy = lx // 2, ly // 2
    for k, (dx, dy) in enumerate(((0, 2), (2, 0), (2, 2), (2, -2), (0, 3), (3, 0), (1, 2), (2, 1))):
        x0, y0 = (cx + 7 * (k - 4)) % lx, (cy + 5 * (k - 4)) % ly
        a, b = (hi, lo) if k % 2 == 0 else (lo, hi)
        if 0 <= x0 - dx and x0 + dx < lx and 0 <= y0 - abs(dy) and y0 + abs(dy) < ly:
            M[x0 - dx, y0 - dy] = a
            M[x0 + dx, y0 + dy] = b
    M[cx, 0] = n          # a grain and the wall at equal distances from the nodes between them
    M[cx, 4] = hi
    out["owner_ties"] = M
    # solid nodes round the wavefront and tile seams
    M = np.full((lx, ly), -1, np.int32)
    k = 0
    for x in (14, 15, 16, 17, 62, 63, 64, 65):
        for y in (14, 15, 16, 17, 62, 63, 64, 65):
            if x < lx and y < ly and (x * 3 + y * 5) % 7 == 0:
                M[x, y] = k % (n + 1)
                k += 1
    out["seam_seeds"] = M
    # random discs
    rng = np.random.default_rng(1000 * lx + ly)
    count = max(3, lx * ly // 850)
    rmax = max(2.0, min(lx, ly) / 12.0)
    out["disc_packing"] = disc_map(lx, ly, [(rng.uniform(0, lx), rng.uniform(0, ly), rng.uniform(1.0, rmax), k % n)
                                            for k in range(count)])
    return out
