"""The pore fluxes restated in numpy (include/lbmdem_hip.h, "Pore fluxes"): per edge of adjacent fluid nodes the mass that crossed
it in the last streaming step as rint(phi * 2^32) in wrapping int64, summed per link and per region of the pore network and per
section of the lattice, the ten counts and the files exactly as the header states them. Every result is an integer sum, so the
device has to reproduce every one of them. restate() is vectorised over network_util.restate; loop() follows the definitions node
by node and shares no code with it."""
import math

import numpy as np

import network_util as nz

NETFLUX_LINK_DTYPE = np.dtype([("flux_q32", np.int64), ("exchange_q32", np.int64), ("edges", np.int64)])
NETFLUX_REGION_DTYPE = np.dtype([("mass_q32", np.int64), ("net_q32", np.int64), ("through_q32", np.int64)])
NETFLUX_COUNTERS = ("fluid_nodes", "regions", "links", "edges", "ridge_edges", "unaccumulated_edges", "unaccumulated_nodes",
                    "flowing_links", "strongest_link", "largest_imbalance")
DATA_HEADER = ("# t fluid_nodes regions links edges ridge_edges unaccumulated_edges unaccumulated_nodes flowing_links strongest_link "
               "largest_imbalance\n")
# an edge's q - p as (dx, dy), the direction i of the population that went from p to q, and its opposite
EDGES = (((0, 1), 8, 4), ((1, -1), 5, 1), ((1, 0), 6, 2), ((1, 1), 7, 3))
Q32 = 4294967296.0
LIMIT = 1048576.0


def quantum(x):
    """(rint(x * 2^32) as int64, left out) elementwise: 0 and left out where x is not finite or |x| >= 2^20"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.abs(x) < LIMIT
    return np.rint(np.where(ok, x, 0.0) * Q32).astype(np.int64), ~ok


def rho_of(f):
    """f0 + f1 + ... + f8, in that order"""
    with np.errstate(invalid="ignore", over="ignore"):
        rho = f[..., 0].copy()
        for q in range(1, 9):
            rho = rho + f[..., q]
    return rho


def region_plane(N, level):
    """the region's index per node, -1 off the fluid; the regions' body numbers"""
    if level == 0:
        return N["body"].astype(np.int64), np.arange(len(N["bodies"]), dtype=np.int64)
    roots = N["groups"]["body"].astype(np.int64)
    g = N["group"].astype(np.int64)
    return np.where(g >= 0, np.searchsorted(roots, np.maximum(g, 0)), -1), roots


def restate(obst, f, n, merge, level, N=None):
    """-> dict(links, regions, col, row, counts, net) of the map obst [lx][ly] and the populations f [lx][ly][9]; N: the
    network_util.restate of (obst, n, merge), where the caller has it"""
    M = np.asarray(obst, dtype=np.int32)
    f = np.asarray(f, dtype=np.float64)
    lx, ly = M.shape
    if N is None:
        N = nz.restate(M, n, merge)
    reg, bodyno = region_plane(N, level)
    table = N["links1" if level else "links0"]
    R, L = len(bodyno), len(table)
    fluid = M == -1
    place = np.full(int(bodyno.max()) + 1 if R else 1, -1, np.int64)   # body number -> region
    place[bodyno] = np.arange(R)
    lo, hi = place[table["lo"]], place[table["hi"]]
    key = lo * max(R, 1) + hi                                          # ascends: the table ascends by (lo, hi)
    links = np.zeros(L, NETFLUX_LINK_DTYPE)
    col, row = np.zeros(lx - 1, np.int64), np.zeros(ly - 1, np.int64)
    edges = ridge = bad_edges = 0
    with np.errstate(over="ignore", invalid="ignore"):
        for (dx, dy), i, opp in EDGES:
            a = (slice(0, lx - dx), slice(max(0, -dy), ly - max(0, dy)))
            b = (slice(dx, lx), slice(max(0, dy), ly - max(0, -dy)))
            m = fluid[a] & fluid[b]
            phi = f[b][..., i] - f[a][..., opp]
            Q, out = quantum(phi)
            Q = np.where(m, Q, 0)
            edges += int(m.sum())
            bad_edges += int((m & out).sum())
            if dx:
                col += Q.sum(axis=1, dtype=np.int64)
            if dy > 0:
                row += Q.sum(axis=0, dtype=np.int64)
            if dy < 0:
                row -= Q.sum(axis=0, dtype=np.int64)   # p in column y + 1, q in column y: Q's column index is q's
            ra, rb = reg[a], reg[b]
            r = m & (ra != rb)
            ridge += int(r.sum())
            if r.any():
                k = np.searchsorted(key, np.minimum(ra, rb)[r] * max(R, 1) + np.maximum(ra, rb)[r])
                sign = np.where(ra[r] < rb[r], 1, -1).astype(np.int64)
                np.add.at(links["flux_q32"], k, sign * Q[r])
                np.add.at(links["exchange_q32"], k, np.abs(Q[r]))
                np.add.at(links["edges"], k, 1)
        mass, out = quantum(rho_of(f))
        regions = np.zeros(R, NETFLUX_REGION_DTYPE)
        np.add.at(regions["mass_q32"], reg[fluid], mass[fluid])
        np.add.at(regions["net_q32"], hi, links["flux_q32"])
        np.subtract.at(regions["net_q32"], lo, links["flux_q32"])
        np.add.at(regions["through_q32"], lo, np.abs(links["flux_q32"]))
        np.add.at(regions["through_q32"], hi, np.abs(links["flux_q32"]))
    counts = dict(zip(NETFLUX_COUNTERS, (
        int(fluid.sum()), R, L, edges, ridge, bad_edges, int((fluid & out).sum()), int((links["flux_q32"] != 0).sum()),
        int(np.argmax(np.abs(links["flux_q32"]))) if L else -1, int(np.abs(regions["net_q32"]).max()) if R else 0)))
    return dict(links=links, regions=regions, col=col, row=row, counts=counts, table=table, region_body=bodyno.astype(np.int32),
                region_nodes=(N["groups"] if level else N["bodies"])["nodes"].astype(np.int64))


def wrap(v):
    """a Python integer as a wrapping int64"""
    return (int(v) + (1 << 63)) % (1 << 64) - (1 << 63)


def loop(obst, f, n, merge, level, N=None):
    """the same node by node in Python integers, from the definitions: small maps only. Also -> node_net, the node-by-node sum
    per region of Q(q -> p) over the nodes' neighbours in another region, and row_in, col_in, the sums per row x (column y) over
    its fluid nodes and their fluid neighbours of Q(q -> p)"""
    M = np.asarray(obst, dtype=np.int32)
    f = np.asarray(f, dtype=np.float64)
    lx, ly = M.shape
    if N is None:
        N = nz.restate(M, n, merge)
    lab = N["group" if level else "body"]
    table = N["links1" if level else "links0"]
    numbers = [int(e["body"]) for e in N["groups"]] if level else list(range(len(N["bodies"])))
    place = {b: i for i, b in enumerate(numbers)}
    where = {(int(e["lo"]), int(e["hi"])): i for i, e in enumerate(table)}
    R, L = len(numbers), len(table)

    def q_of(x):
        x = float(x)
        if math.isnan(x) or math.isinf(x) or not abs(x) < LIMIT:
            return 0, 1
        return int(round(x * Q32)), 0   # (Python's round on a float is to even, as rint)

    flux, exch, cnt = [0] * L, [0] * L, [0] * L
    mass, node_net = [0] * R, [0] * R
    col, row = [0] * (lx - 1), [0] * (ly - 1)
    row_in, col_in = [0] * lx, [0] * ly
    fluid_nodes = edges = ridge = bad_e = bad_n = 0
    for x in range(lx):
        for y in range(ly):
            if M[x, y] != -1:
                continue
            fluid_nodes += 1
            rho = f[x, y, 0]
            with np.errstate(invalid="ignore", over="ignore"):
                for q in range(1, 9):
                    rho = rho + f[x, y, q]
            m, bad = q_of(rho)
            bad_n += bad
            mass[place[int(lab[x, y])]] += m
            for (dx, dy), i, opp in EDGES:
                xq, yq = x + dx, y + dy
                if xq >= lx or yq < 0 or yq >= ly or M[xq, yq] != -1:
                    continue
                edges += 1
                with np.errstate(invalid="ignore", over="ignore"):
                    Q, bad = q_of(f[xq, yq, i] - f[x, y, opp])
                bad_e += bad
                if dx:
                    col[x] += Q
                    row_in[x] -= Q
                    row_in[xq] += Q
                if dy > 0:
                    row[y] += Q
                if dy < 0:
                    row[yq] -= Q
                if dy:
                    col_in[y] -= Q
                    col_in[yq] += Q
                a, b = int(lab[x, y]), int(lab[xq, yq])
                if a != b:
                    ridge += 1
                    k = where[(min(a, b), max(a, b))]
                    flux[k] += Q if a < b else -Q
                    exch[k] += abs(Q)
                    cnt[k] += 1
                    node_net[place[a]] -= Q
                    node_net[place[b]] += Q
    net, through = [0] * R, [0] * R
    for k, e in enumerate(table):
        a, b = place[int(e["lo"])], place[int(e["hi"])]
        net[b] += flux[k]
        net[a] -= flux[k]
        through[a] += abs(flux[k])
        through[b] += abs(flux[k])
    links = np.zeros(L, NETFLUX_LINK_DTYPE)
    regions = np.zeros(R, NETFLUX_REGION_DTYPE)
    links["flux_q32"], links["exchange_q32"], links["edges"] = [wrap(v) for v in flux], [wrap(v) for v in exch], cnt
    regions["mass_q32"], regions["net_q32"], regions["through_q32"] = ([wrap(v) for v in mass], [wrap(v) for v in net],
                                                                        [wrap(v) for v in through])
    strongest = -1
    for k in range(L):
        if strongest < 0 or abs(flux[k]) > abs(flux[strongest]):
            strongest = k
    counts = dict(zip(NETFLUX_COUNTERS, (fluid_nodes, R, L, edges, ridge, bad_e, bad_n, sum(1 for v in flux if v), strongest,
                                         max([abs(v) for v in net], default=0))))
    return dict(links=links, regions=regions, col=np.array([wrap(v) for v in col], np.int64).reshape(-1),
                row=np.array([wrap(v) for v in row], np.int64).reshape(-1), counts=counts, table=table,
                region_body=np.array(numbers, np.int32), region_nodes=(N["groups"] if level else N["bodies"])["nodes"].astype(np.int64),
                node_net=node_net, row_in=row_in, col_in=col_in)


def same(D, W):
    """every output of two statements (or of the device and one) equal -> the name of the first that differs, or None"""
    if D["counts"] != W["counts"]:
        return "counts"
    for name in ("col", "row"):
        if not np.array_equal(D[name], W[name]):
            return name
    for name, dt in (("links", NETFLUX_LINK_DTYPE), ("regions", NETFLUX_REGION_DTYPE)):
        if len(D[name]) != len(W[name]):
            return name
        for fld in dt.names:
            if not np.array_equal(D[name][fld], W[name][fld]):
                return name + "." + fld
    return None


def files_bytes(lx, ly, n, merge, level, W, t, nfile=0):
    """the files of lbmdem_write_netflux_files as the header spells them out -> {name: bytes}; netflux.data: the one line"""
    first = "# lx %d ly %d n %d merge %d level %d\n" % (lx, ly, n, merge, level)
    li = [first, "# lo hi edges saddle flux_q32 exchange_q32\n"]
    for e, v in zip(W["table"], W["links"]):
        li.append("%d %d %d %d %d %d\n" % (e["lo"], e["hi"], v["edges"], e["saddle"], v["flux_q32"], v["exchange_q32"]))
    rg = [first, "# region body nodes mass_q32 net_q32 through_q32\n"]
    for k, v in enumerate(W["regions"]):
        rg.append("%d %d %d %d %d %d\n" % (k, W["region_body"][k], W["region_nodes"][k], v["mass_q32"], v["net_q32"], v["through_q32"]))
    pr = [first, "# axis index flux_q32\n"]
    pr += ["x %d %d\n" % (x, v) for x, v in enumerate(W["col"])]
    pr += ["y %d %d\n" % (y, v) for y, v in enumerate(W["row"])]
    line = "%e" % t + "".join(" %d" % W["counts"][k] for k in NETFLUX_COUNTERS) + "\n"
    return {"netflux_links%06d.dat" % nfile: "".join(li).encode(), "netflux_regions%06d.dat" % nfile: "".join(rg).encode(),
            "netflux_profile%06d.dat" % nfile: "".join(pr).encode(), "netflux.data": line.encode()}
