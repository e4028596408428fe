"""The pore space analysis restated in numpy (include/lbmdem_hip.h, "Pore space"): the fluid nodes of a map [lx][ly] labelled into
components by a union-find, the table, the per-grain outputs and the ten counts exactly as the header states them -- every result is
an integer, so the device has to reproduce every one of them. And the maps the tests label: the shapes a tiled union-find gets
wrong."""
import numpy as np

PORE_DTYPE = np.dtype([("label", np.int32), ("walls", np.int32), ("nodes", np.int64), ("grain_links", np.int64),
                       ("wall_links", np.int64), ("mass_q32", np.int64), ("xmin", np.int32), ("xmax", np.int32), ("ymin", np.int32),
                       ("ymax", np.int32)])
PORE_COUNTERS = ("fluid_nodes", "components", "largest_nodes", "largest_label", "trapped_nodes", "single_nodes", "spanning",
                 "throat_grains", "dry_grains", "unaccumulated")
# the directions q = 0..8 (main.c:70-71)
EX = (0, -1, -1, -1, 0, 1, 1, 1, 0)
EY = (0, 1, 0, -1, -1, -1, 0, 1, 1)
DATA_HEADER = ("# t fluid_nodes components largest_nodes largest_label trapped_nodes single_nodes spanning throat_grains dry_grains "
               "unaccumulated\n")


def components(M, conn):
    """label[lx][ly] int32: the smallest index x * ly + y of a fluid node's component, -1 off the fluid. A union-find over the
    edge list: every round hooks the larger root of an edge below the smaller and halves the paths until nothing moves."""
    assert conn in (4, 8)
    M = np.asarray(M)
    lx, ly = M.shape
    fluid = M == -1
    idx = np.arange(lx * ly, dtype=np.int64).reshape(lx, ly)
    ea, eb = [], []
    for dx, dy in ((1, 0), (0, 1)) + (((1, 1), (1, -1)) if conn == 8 else ()):
        a = (slice(0, lx - dx), slice(max(0, -dy), ly - max(0, dy)))
        b = (slice(dx, lx), slice(max(0, dy), ly - max(0, -dy)))
        both = fluid[a] & fluid[b]
        ea.append(idx[a][both]); eb.append(idx[b][both])
    ea, eb = np.concatenate(ea), np.concatenate(eb)
    P = np.arange(lx * ly, dtype=np.int64)
    while True:
        ra, rb = P[ea], P[eb]
        hi, lo = np.maximum(ra, rb), np.minimum(ra, rb)
        m = hi != lo
        if not m.any():
            break
        np.minimum.at(P, hi[m], lo[m])
        while True:
            Q = P[P]
            if np.array_equal(Q, P):
                break
            P = Q
    return np.where(fluid, P.reshape(lx, ly), -1).astype(np.int32)


def rho_of(f):
    """lbmdem_download_macro's rho: 0. + f0 + .. + f8, in that order"""
    rho = np.zeros(f.shape[:2])
    for q in range(9):
        rho = rho + f[:, :, q]
    return rho


def restate(M, f, n, conn):
    """-> dict(label, table, wet, pore_min, pore_max, counts) of the map M [lx][ly] (-1 fluid, 0 .. n - 1 a grain, n the wall), the
    populations f [lx][ly][9] and the grain count"""
    M = np.asarray(M, dtype=np.int32)
    lx, ly = M.shape
    label = components(M, conn)
    fluid = M == -1
    X, Y = np.meshgrid(np.arange(lx), np.arange(ly), indexing="ij")
    Mp = np.full((lx + 2, ly + 2), n, np.int32)        # outside the lattice: as a wall node
    Mp[1:-1, 1:-1] = M
    Lp = np.full((lx + 2, ly + 2), -1, np.int64)       # outside the lattice: no fluid
    Lp[1:-1, 1:-1] = label
    glinks, wlinks, walls = (np.zeros((lx, ly), np.int64) for _ in range(3))
    wet = np.zeros(n, np.int64)
    pmin, pmax = np.full(n, np.iinfo(np.int64).max), np.full(n, -1, np.int64)
    grain = (M >= 0) & (M < n)
    for q in range(1, 9):
        nb = Mp[1 + EX[q]:1 + EX[q] + lx, 1 + EY[q]:1 + EY[q] + ly]
        nl = Lp[1 + EX[q]:1 + EX[q] + lx, 1 + EY[q]:1 + EY[q] + ly]
        nx, ny = X + EX[q], Y + EY[q]
        glinks += (nb >= 0) & (nb < n)
        w = nb == n
        wlinks += w
        walls |= np.where(w, (ny <= 0) * 1 | (ny >= ly - 1) * 2 | (nx <= 0) * 4 | (nx >= lx - 1) * 8, 0)
        g = grain & (nl >= 0)
        np.add.at(wet, M[g], 1)
        np.minimum.at(pmin, M[g], nl[g])
        np.maximum.at(pmax, M[g], nl[g])
    pmin[pmin == np.iinfo(np.int64).max] = -1
    rho = rho_of(np.asarray(f, dtype=np.float64))
    with np.errstate(invalid="ignore", over="ignore"):
        ok = np.isfinite(rho) & (np.abs(rho) < 2.0 ** 20)
        q32 = np.where(ok, np.rint(np.where(ok, rho, 0.0) * 4294967296.0), 0.0).astype(np.int64)
    labels, inv = np.unique(label[fluid], return_inverse=True)
    table = np.zeros(len(labels), PORE_DTYPE)
    table["label"] = labels
    table["xmin"] = table["ymin"] = np.iinfo(np.int32).max
    table["xmax"] = table["ymax"] = -1
    if len(labels):
        table["nodes"] = np.bincount(inv, minlength=len(labels))
        for name, plane in (("grain_links", glinks), ("wall_links", wlinks), ("mass_q32", q32)):
            acc = np.zeros(len(labels), np.int64)
            np.add.at(acc, inv, plane[fluid])      # (int64 wraps)
            table[name] = acc
        acc = np.zeros(len(labels), np.int64)
        np.bitwise_or.at(acc, inv, walls[fluid])
        table["walls"] = acc
        for name, plane, op in (("xmin", X, np.minimum), ("xmax", X, np.maximum), ("ymin", Y, np.minimum), ("ymax", Y, np.maximum)):
            acc = table[name].astype(np.int64)
            op.at(acc, inv, plane[fluid])
            table[name] = acc
    nodes = table["nodes"]
    big = int(np.argmax(nodes)) if len(nodes) else -1      # (argmax: the first among equals, the smallest label)
    span = 0
    if ((table["walls"] & 12) == 12).any():
        span |= 1
    if ((table["walls"] & 3) == 3).any():
        span |= 2
    counts = dict(zip(PORE_COUNTERS, (int(fluid.sum()), len(labels), int(nodes[big]) if big >= 0 else 0,
                                      int(labels[big]) if big >= 0 else -1, int(fluid.sum()) - (int(nodes[big]) if big >= 0 else 0),
                                      int((nodes == 1).sum()), span, int((pmin != pmax).sum()), int((wet == 0).sum()),
                                      int((fluid & ~ok).sum()))))
    return dict(label=label, table=table, wet=wet.astype(np.int32), pore_min=pmin.astype(np.int32), pore_max=pmax.astype(np.int32),
                counts=counts)


def files_bytes(conn, lx, ly, R, t, nfile=0, plane=False):
    """the files of lbmdem_write_pore_files as the header spells them out -> {name: bytes}; pores.data: the one line"""
    tab = ["# conn %d lx %d ly %d\n" % (conn, lx, ly), "# label nodes xmin xmax ymin ymax grain_links wall_links walls mass_q32\n"]
    for e in R["table"]:
        tab.append("%d %d %d %d %d %d %d %d %d %d\n" % (e["label"], e["nodes"], e["xmin"], e["xmax"], e["ymin"], e["ymax"],
                                                       e["grain_links"], e["wall_links"], e["walls"], e["mass_q32"]))
    gr = ["# i wet pore_min pore_max\n"]
    for i in range(len(R["wet"])):
        gr.append("%d %d %d %d\n" % (i, R["wet"][i], R["pore_min"][i], R["pore_max"][i]))
    line = "%e" % t + "".join(" %d" % R["counts"][k] for k in PORE_COUNTERS) + "\n"
    out = {"pore_table%06d.dat" % nfile: "".join(tab).encode(), "pore_grains%06d.dat" % nfile: "".join(gr).encode(),
           "pores.data": line.encode()}
    if plane:
        pas = float(np.float32(1.0 / lx))
        head = ("# vtk DataFile Version 2.0\nlbmdem pore labels\nBINARY\nDATASET STRUCTURED_POINTS\n"
                "DIMENSIONS %d %d 1\nORIGIN 0 0 0\nSPACING %.9g %.9g 1\n"
                "POINT_DATA %d\nSCALARS pore int 1\nLOOKUP_TABLE default\n" % (lx, ly, pas, pas, lx * ly))
        out["pores%06d.vtk" % nfile] = head.encode() + np.ascontiguousarray(R["label"].T).astype(">i4").tobytes()
    return out


# ---- the maps ----

def solid_values(lx, ly, n):
    """what the nodes off the fluid hold: grains and wall nodes mixed, so that the grain outputs and both kinds of links are used"""
    X, Y = np.meshgrid(np.arange(lx), np.arange(ly), indexing="ij")
    return ((X * 7 + Y * 13) % (n + 1)).astype(np.int32)


def with_fluid(fluid, n):
    lx, ly = fluid.shape
    return np.where(fluid, -1, solid_values(lx, ly, n)).astype(np.int32)


def shape_maps(lx, ly, n):
    """name -> map [lx][ly]: the cases of a tiled union-find"""
    X, Y = np.meshgrid(np.arange(lx), np.arange(ly), indexing="ij")
    out = {}
    out["all_fluid"] = np.ones((lx, ly), bool)
    out["no_fluid"] = np.zeros((lx, ly), bool)
    one = np.zeros((lx, ly), bool)
    one[lx // 2, ly - 1] = True
    out["one_node"] = one
    out["checkerboard"] = (X + Y) % 2 == 0
    out["antidiagonal_stripes"] = (X + Y) % 3 == 0              # only 8 joins the nodes of a stripe
    # corridors along y in every other row, joined at alternating ends: one path of about lx * ly / 2 nodes
    s = X % 2 == 0
    gap_hi = (X % 4 == 1) & (Y == ly - 1)
    gap_lo = (X % 4 == 3) & (Y == 0)
    out["serpentine"] = s | gap_hi | gap_lo
    # a square spiral: every other ring is fluid; ring k is cut at (k, k + 1), next to where the door (k + 1, k + 2) leads on
    # into ring k + 2, so that the way in from (k, k) runs once round the ring
    ring = np.minimum(np.minimum(X, lx - 1 - X), np.minimum(Y, ly - 1 - Y))
    sp = ring % 2 == 0
    for k in range(0, min(lx, ly) // 2 - 3, 2):
        sp[k, k + 1] = False
        sp[k + 1, k + 2] = True
    out["spiral"] = sp
    # a comb: teeth along y in every other row, joined only in the last column
    out["comb"] = ((X % 2 == 0) & (Y < ly - 1)) | (Y == ly - 1)
    # a U: two arms that start in different tiles (rows 1 and lx - 2) and meet in the last column only
    u = np.zeros((lx, ly), bool)
    u[1, 1:] = True
    u[lx - 2, 1:] = True
    u[1:lx - 1, ly - 1] = True
    out["u_shape"] = u
    for frac, seed in ((0.4, 11), (0.6, 12), (0.8, 13)):
        out["random_%02d" % int(frac * 100)] = np.random.default_rng(seed).random((lx, ly)) < frac
    return {k: with_fluid(v, n) for k, v in out.items()}
