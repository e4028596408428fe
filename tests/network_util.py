"""The pore network restated in numpy (include/lbmdem_hip.h, "Pore network"): a watershed of the clearance analysis' exact squared
distance d2 -- every fluid node climbs to the local maximum it belongs to --, the bodies, the links between adjacent basins with
their saddles, one round of merging and the same links between the merged groups, the ten counts and the files exactly as the
header states them. Every result is an integer and every tie has a rule, so the device has to reproduce every one of them.
restate() is vectorised; brute_force() follows the definitions node by node."""
import numpy as np

import clearance_util as cz

NET_BODY_DTYPE = np.dtype([("node", np.int32), ("d2", np.int32), ("nodes", np.int64), ("degree", np.int32), ("parent", np.int32),
                           ("group", np.int32)], align=True)
NET_LINK_DTYPE = np.dtype([("lo", np.int32), ("hi", np.int32), ("edges", np.int32), ("saddle", np.int32), ("node", np.int32)])
NET_GROUP_DTYPE = np.dtype([("body", np.int32), ("bodies", np.int32), ("nodes", np.int64), ("d2", np.int32), ("node", np.int32),
                            ("degree", np.int32)], align=True)
NETWORK_COUNTERS = ("fluid_nodes", "bodies", "body_links", "body_edges", "groups", "group_links", "group_edges", "isolated_groups",
                    "largest_group_nodes", "narrowest_saddle")
DATA_HEADER = ("# t fluid_nodes bodies body_links body_edges groups group_links group_edges isolated_groups largest_group_nodes "
               "narrowest_saddle\n")
# q - p of an edge's two nodes p < q, as (dx, dy): p + 1, p + ly - 1, p + ly, p + ly + 1
STEPS = ((0, 1), (1, -1), (1, 0), (1, 1))


def links_of(lab, d2):
    """rule 3 over the label plane lab (-1 off the fluid) -> (table of NET_LINK_DTYPE, number of edges)"""
    lx, ly = lab.shape
    idx = np.arange(lx * ly, dtype=np.int64).reshape(lx, ly)
    lo, hi, s, p = [], [], [], []
    for dx, dy in STEPS:
        a = (slice(0, lx - dx), slice(max(0, -dy), ly - max(0, dy)))
        b = (slice(dx, lx), slice(max(0, dy), ly - max(0, -dy)))
        m = (lab[a] >= 0) & (lab[b] >= 0) & (lab[a] != lab[b])
        lo.append(np.minimum(lab[a], lab[b])[m]); hi.append(np.maximum(lab[a], lab[b])[m])
        s.append(np.minimum(d2[a], d2[b])[m]); p.append(idx[a][m])
    lo, hi, s, p = (np.concatenate(v).astype(np.int64) for v in (lo, hi, s, p))
    order = np.lexsort((p, -s, hi, lo))
    lo, hi, s, p = lo[order], hi[order], s[order], p[order]
    head = np.ones(len(lo), bool)
    head[1:] = (lo[1:] != lo[:-1]) | (hi[1:] != hi[:-1])
    first = np.nonzero(head)[0]
    table = np.zeros(len(first), NET_LINK_DTYPE)
    table["lo"], table["hi"], table["saddle"], table["node"] = lo[first], hi[first], s[first], p[first]
    table["edges"] = np.diff(np.append(first, len(lo)))
    return table, len(lo)


def degrees(table, count):
    return (np.bincount(table["lo"], minlength=count) + np.bincount(table["hi"], minlength=count)).astype(np.int32)


def merged(bnode, bd2, links, merge):
    """rule 4 -> (parent, group) per body"""
    B = len(bnode)
    parent = np.arange(B, dtype=np.int64)
    if merge >= 0 and len(links):
        a = np.concatenate([links["lo"], links["hi"]]).astype(np.int64)
        b = np.concatenate([links["hi"], links["lo"]]).astype(np.int64)
        s = np.concatenate([links["saddle"], links["saddle"]]).astype(np.int64)
        higher = (bd2[b] > bd2[a]) | ((bd2[b] == bd2[a]) & (bnode[b] < bnode[a]))
        ok = higher & (cz.isqrt(bd2[a]) - cz.isqrt(s) <= merge)
        a, b, s = a[ok], b[ok], s[ok]
        order = np.lexsort((b, -s, a))
        a, b = a[order], b[order]
        head = np.ones(len(a), bool)
        head[1:] = a[1:] != a[:-1]
        parent[a[head]] = b[head]
    group = parent.copy()
    while True:
        nxt = group[group]
        if np.array_equal(nxt, group):
            break
        group = nxt
    return parent.astype(np.int32), group.astype(np.int32)


def finish(M, d2, body, merge):
    """everything behind rule 2's plane: records, links of both levels, merge, groups, counts"""
    fluid = body >= 0
    lx, ly = body.shape
    flat = body.reshape(-1)
    B = int(flat.max()) + 1 if fluid.any() else 0
    k = np.nonzero(flat >= 0)[0]
    d2f = d2.reshape(-1).astype(np.int64)
    best = np.full(B, -1, np.int64)          # a body's peak is its highest node
    np.maximum.at(best, flat[k], (d2f[k] << 32) | (lx * ly - 1 - k))
    bnode = lx * ly - 1 - (best & 0xFFFFFFFF)
    bd2 = best >> 32
    links0, edges0 = links_of(body, d2)
    parent, grp = merged(bnode, bd2, links0, merge)
    bodies = np.zeros(B, NET_BODY_DTYPE)
    bodies["node"], bodies["d2"] = bnode, bd2
    bodies["nodes"] = np.bincount(flat[k], minlength=B)
    bodies["degree"] = degrees(links0, B)
    bodies["parent"], bodies["group"] = parent, grp
    group = np.where(fluid, grp[np.where(fluid, body, 0)] if B else -1, -1).astype(np.int32)
    links1, edges1 = links_of(group, d2)
    roots = np.nonzero(grp == np.arange(B))[0]
    groups = np.zeros(len(roots), NET_GROUP_DTYPE)
    groups["body"] = roots
    groups["bodies"] = np.bincount(grp, minlength=B)[roots] if B else 0
    groups["nodes"] = np.bincount(grp, weights=bodies["nodes"], minlength=B)[roots].astype(np.int64) if B else 0
    groups["d2"], groups["node"] = bodies["d2"][roots], bodies["node"][roots]
    groups["degree"] = degrees(links1, B)[roots] if B else 0
    counts = dict(zip(NETWORK_COUNTERS, (int(fluid.sum()), B, len(links0), edges0, len(roots), len(links1), edges1,
                                         int((groups["degree"] == 0).sum()), int(groups["nodes"].max()) if len(roots) else 0,
                                         int(links1["saddle"].min()) if len(links1) else -1)))
    return dict(d2=d2, body=body, group=group, bodies=bodies, groups=groups, links0=links0, links1=links1, counts=counts)


def restate(M, n, merge):
    """-> dict(d2, body, group, bodies, groups, links0, links1, counts) of the map M [lx][ly] (-1 fluid, 0 .. n - 1 a grain, n the
    wall) over clearance_util.restate's d2"""
    return finish_from(M, cz.restate(M, n)["d2"], merge)


def finish_from(M, d2, merge):
    """rules 1 to 7 over a given d2 plane"""
    M = np.asarray(M, dtype=np.int32)
    lx, ly = M.shape
    N = lx * ly
    fluid = M == -1
    idx = np.arange(N, dtype=np.int64).reshape(lx, ly)
    key = np.where(fluid, (d2.astype(np.int64) << 32) | (N - 1 - idx), -1)
    K = np.full((lx + 2, ly + 2), -1, np.int64)
    K[1:-1, 1:-1] = key
    top = key.copy()
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            top = np.maximum(top, K[1 + dx:1 + dx + lx, 1 + dy:1 + dy + ly])
    up = np.where(fluid, N - 1 - (top & 0xFFFFFFFF), idx).reshape(-1)
    while True:
        nxt = up[up]
        if np.array_equal(nxt, up):
            break
        up = nxt
    peak = up.reshape(lx, ly)
    peaks = np.unique(peak[fluid])
    body = np.where(fluid, np.searchsorted(peaks, peak), -1).astype(np.int32)
    return finish(M, d2, body, merge)


def brute_force(M, n, merge):
    """the same by loops that follow the definitions literally: small maps only"""
    M = np.asarray(M, dtype=np.int32)
    lx, ly = M.shape
    N = lx * ly
    d2 = (cz.brute_force(M, n) >> 32).astype(np.int32) * (M == -1)
    D = d2.reshape(-1)
    F = (M == -1).reshape(-1)

    def adjacent(p):
        x, y = divmod(p, ly)
        return [(x + dx) * ly + y + dy for dx in (-1, 0, 1) for dy in (-1, 0, 1)
                if (dx or dy) and 0 <= x + dx < lx and 0 <= y + dy < ly and F[(x + dx) * ly + y + dy]]

    def higher(p, q):
        return D[p] > D[q] or (D[p] == D[q] and p < q)

    def up(p):
        best = p
        for q in adjacent(p):
            if higher(q, best):
                best = q
        return best

    peak_of = {}
    for p in range(N):
        if F[p]:
            q = p
            while up(q) != q:
                q = up(q)
            peak_of[p] = q
    peaks = sorted(set(peak_of.values()))
    number = {q: i for i, q in enumerate(peaks)}
    body = np.full(N, -1, np.int32)
    for p, q in peak_of.items():
        body[p] = number[q]

    def links(lab):
        found = {}
        edges = 0
        for p in range(N):
            if lab[p] < 0:
                continue
            for q in adjacent(p):
                if q > p and lab[q] != lab[p]:
                    edges += 1
                    pair = (min(lab[p], lab[q]), max(lab[p], lab[q]))
                    h = min(D[p], D[q])
                    e = found.setdefault(pair, [0, -1, -1])
                    e[0] += 1
                    if h > e[1]:
                        e[1], e[2] = h, p
                    # (p ascends: the first node of a height is its smallest)
        table = np.zeros(len(found), NET_LINK_DTYPE)
        for i, pair in enumerate(sorted(found)):
            table[i] = (pair[0], pair[1], found[pair][0], found[pair][1], found[pair][2])
        return table, edges

    links0, edges0 = links(body)
    B = len(peaks)
    parent = list(range(B))
    if merge >= 0:
        for a in range(B):
            best = None
            for e in links0:
                if a not in (e["lo"], e["hi"]):
                    continue
                b = int(e["hi"] if e["lo"] == a else e["lo"])
                if not higher(peaks[b], peaks[a]):
                    continue
                if int(cz.isqrt(D[peaks[a]])) - int(cz.isqrt(e["saddle"])) > merge:
                    continue
                if best is None or e["saddle"] > best[0] or (e["saddle"] == best[0] and b < best[1]):
                    best = (int(e["saddle"]), b)
            if best is not None:
                parent[a] = best[1]
    grp = []
    for a in range(B):
        while parent[a] != a:
            a = parent[a]
        grp.append(a)
    group = np.array([grp[b] if b >= 0 else -1 for b in body], np.int32)
    links1, edges1 = links(group)
    bodies = np.zeros(B, NET_BODY_DTYPE)
    for a in range(B):
        deg = sum(1 for e in links0 if a in (e["lo"], e["hi"]))
        bodies[a] = (peaks[a], D[peaks[a]], int((body == a).sum()), deg, parent[a], grp[a])
    roots = [a for a in range(B) if grp[a] == a]
    groups = np.zeros(len(roots), NET_GROUP_DTYPE)
    for i, a in enumerate(roots):
        deg = sum(1 for e in links1 if a in (e["lo"], e["hi"]))
        groups[i] = (a, grp.count(a), int((group == a).sum()), D[peaks[a]], peaks[a], deg)
    counts = dict(zip(NETWORK_COUNTERS, (int(F.sum()), B, len(links0), edges0, len(roots), len(links1), edges1,
                                         int((groups["degree"] == 0).sum()), int(groups["nodes"].max()) if roots else 0,
                                         int(links1["saddle"].min()) if len(links1) else -1)))
    return dict(d2=d2, body=body.reshape(lx, ly), group=group.reshape(lx, ly), bodies=bodies, groups=groups, links0=links0,
                links1=links1, counts=counts)


def same(A, B):
    """every output of two restatements (or of the device and one) equal -> the name of the first that differs, or None"""
    if A["counts"] != B["counts"]:
        return "counts"
    for name in ("body", "group"):
        if not np.array_equal(A[name], B[name]):
            return name
    for name, dt in (("bodies", NET_BODY_DTYPE), ("groups", NET_GROUP_DTYPE), ("links0", NET_LINK_DTYPE), ("links1", NET_LINK_DTYPE)):
        if len(A[name]) != len(B[name]):
            return name
        for f in dt.names:
            if not np.array_equal(A[name][f], B[name][f]):
                return name + "." + f
    return None


def files_bytes(lx, ly, n, merge, R, t, nfile=0, plane=False):
    """the files of lbmdem_write_network_files as the header spells them out -> {name: bytes}; network.data: the one line"""
    bo = ["# lx %d ly %d n %d merge %d\n" % (lx, ly, n, merge), "# body node d2 nodes degree parent group\n"]
    for i, e in enumerate(R["bodies"]):
        bo.append("%d %d %d %d %d %d %d\n" % (i, e["node"], e["d2"], e["nodes"], e["degree"], e["parent"], e["group"]))
    li = ["# lx %d ly %d n %d merge %d\n" % (lx, ly, n, merge), "# lo hi edges saddle node\n"]
    for e in R["links1"]:
        li.append("%d %d %d %d %d\n" % (e["lo"], e["hi"], e["edges"], e["saddle"], e["node"]))
    gr = ["# lx %d ly %d n %d merge %d\n" % (lx, ly, n, merge), "# body bodies nodes d2 node degree\n"]
    for e in R["groups"]:
        gr.append("%d %d %d %d %d %d\n" % (e["body"], e["bodies"], e["nodes"], e["d2"], e["node"], e["degree"]))
    line = "%e" % t + "".join(" %d" % R["counts"][k] for k in NETWORK_COUNTERS) + "\n"
    out = {"network_bodies%06d.dat" % nfile: "".join(bo).encode(), "network_links%06d.dat" % nfile: "".join(li).encode(),
           "network_groups%06d.dat" % nfile: "".join(gr).encode(), "network.data": line.encode()}
    if plane:
        pas = float(np.float32(1.0 / lx))
        data = ("# vtk DataFile Version 2.0\nlbmdem pore network\nBINARY\nDATASET STRUCTURED_POINTS\n"
                "DIMENSIONS %d %d 1\nORIGIN 0 0 0\nSPACING %.9g %.9g 1\nPOINT_DATA %d\n" % (lx, ly, pas, pas, lx * ly)).encode()
        for name in ("body", "group"):
            data += ("SCALARS %s int 1\nLOOKUP_TABLE default\n" % name).encode()
            data += np.ascontiguousarray(R[name].T).astype(">i4").tobytes() + b"\n"
        out["network%06d.vtk" % nfile] = data
    return out
