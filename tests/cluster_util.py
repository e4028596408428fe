"""Shared by the cluster analysis tests (tests/test_cluster_host.py, tests/test_gpu_clusters.py): a plain-Python / numpy
restatement of include/lbmdem_hip.h's "Force chains" block from a record list (contacts_util.CONTACT_DTYPE, the order of
lbmdem_download_contacts) and the grains' centres, and the text of the four files of lbmdem_write_clusters_files.

Everything but the threshold is an integer or a minimum / maximum; the threshold's sum S is the chain the header spells out:
pair records in record order, blocks of 1024, each block added serially from +0.0, then the partials added serially."""
import numpy as np

from contacts_util import CONTACT_DTYPE, WALL_B, WALL_L, WALL_R, WALL_T

CLUSTER_DTYPE = np.dtype([("label", np.int32), ("size", np.int32), ("contacts", np.int64), ("walls", np.int32), ("core", np.int32),
                          ("xmin", np.float64), ("xmax", np.float64), ("ymin", np.float64), ("ymax", np.float64)])
COUNTERS = ("selected_pairs", "selected_walls", "clusters", "largest_size", "largest_label", "isolated_grains", "core_grains",
            "core_pairs", "core_walls", "spanning")
BLOCK = 1024
PALETTE = ("0.894 0.102 0.110", "0.216 0.494 0.722", "0.302 0.686 0.290", "0.596 0.306 0.639", "1.000 0.498 0.000",
           "0.651 0.337 0.157", "0.969 0.506 0.749", "0.400 0.400 0.400")
DATA_HEADER = ("# t threshold selected_pairs selected_walls clusters largest_size largest_label isolated_grains core_grains "
               "core_pairs core_walls spanning\n")


def s_chain(fn):
    """(S, m) over the pair records' fn in record order: Python floats are IEEE doubles, every += is one rounded addition"""
    S, m = 0.0, 0
    for b in range(0, len(fn), BLOCK):
        part = 0.0
        for v in fn[b:b + BLOCK]:
            v = float(v)
            if v > 0:
                part += v
                m += 1
        S += part
    return S, m


def threshold(rec, fmin, relative):
    fmin = float(fmin)
    if not relative:
        return fmin
    S, m = s_chain(rec["fn"][rec["j"] >= 0])
    if m == 0:
        return float("inf") if fmin > 0 else 0.0
    return fmin * (S / float(m))


def order_key(v):
    """doubles as integers of the same order: -0.0 below +0.0, a NaN beyond the infinity of its sign"""
    b = np.ascontiguousarray(v, np.float64).view(np.uint64)
    neg = (b >> np.uint64(63)) != 0
    return np.where(neg, ~b, b | np.uint64(1 << 63))


def labels_union_find(n, pairs):
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for i, j in pairs:
        a, b = find(int(i)), find(int(j))
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(i) for i in range(n)], np.int32)


def core_sweeps(n, pairs, wall_count, zmin):
    """the naive repeated sweep: every grain whose remaining degree is below zmin goes, all at once, until a sweep removes
    nothing -> (core, sweeps that removed something)"""
    alive = np.ones(n, bool)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    rounds = 0
    while True:
        rem = np.asarray(wall_count, np.int64).copy()
        both = alive[pairs[:, 0]] & alive[pairs[:, 1]]
        np.add.at(rem, pairs[both, 0], 1)
        np.add.at(rem, pairs[both, 1], 1)
        out = alive & (rem < zmin)
        if not out.any():
            return alive.astype(np.int32), rounds
        alive &= ~out
        rounds += 1


def restate(rec, n, x1, x2, fmin, relative, zmin):
    """-> dict: thr, sel (per record), label, degree, core, walls (per grain), table (CLUSTER_DTYPE), counts (dict of COUNTERS),
    peel_rounds"""
    rec = np.ascontiguousarray(rec, CONTACT_DTYPE)
    thr = threshold(rec, fmin, relative)
    sel = rec["fn"] >= thr                      # (False for NaN)
    ispair = rec["j"] >= 0
    sp, sw = rec[sel & ispair], rec[sel & ~ispair]
    degree = np.zeros(n, np.int32)
    walls = np.zeros(n, np.int32)
    wall_count = np.zeros(n, np.int64)
    for c in sp:
        degree[c["i"]] += 1
        degree[c["j"]] += 1
    for c in sw:
        degree[c["i"]] += 1
        wall_count[c["i"]] += 1
        walls[c["i"]] |= 1 << (-int(c["j"]) - 1)
    pairs = np.stack([sp["i"], sp["j"]], axis=1).astype(np.int64) if len(sp) else np.zeros((0, 2), np.int64)
    label = labels_union_find(n, pairs)
    core, peel_rounds = core_sweeps(n, pairs, wall_count, zmin)
    kx, ky = order_key(x1), order_key(x2)
    x1, x2 = np.asarray(x1, np.float64), np.asarray(x2, np.float64)
    rows = []
    for L in sorted(set(label.tolist())):
        mem = np.nonzero(label == L)[0]
        if len(mem) < 2:
            continue
        rows.append((L, len(mem), int((label[sp["i"]] == L).sum()), int(np.bitwise_or.reduce(walls[mem])), int(core[mem].sum()),
                     x1[mem[np.argmin(kx[mem])]], x1[mem[np.argmax(kx[mem])]], x2[mem[np.argmin(ky[mem])]],
                     x2[mem[np.argmax(ky[mem])]]))
    table = np.array(rows, CLUSTER_DTYPE) if rows else np.zeros(0, CLUSTER_DTYPE)
    sizes = np.bincount(label, minlength=n)
    largest = int(sizes.max())
    comp_walls = np.zeros(n, np.int64)
    np.bitwise_or.at(comp_walls, label, walls)
    lr, bt = (1 << (-WALL_L - 1)) | (1 << (-WALL_R - 1)), (1 << (-WALL_B - 1)) | (1 << (-WALL_T - 1))
    span = (1 if ((comp_walls & lr) == lr).any() else 0) | (2 if ((comp_walls & bt) == bt).any() else 0)
    counts = dict(zip(COUNTERS, (len(sp), len(sw), len(table), largest, int(np.nonzero(sizes == largest)[0][0]),
                                 int((degree == 0).sum()), int(core.sum()),
                                 int((core[sp["i"]] & core[sp["j"]]).sum()) if len(sp) else 0,
                                 int(core[sw["i"]].sum()) if len(sw) else 0, span)))
    return dict(thr=thr, sel=sel, label=label, degree=degree, core=core, walls=walls, table=table, counts=counts,
                peel_rounds=peel_rounds)


def same_bits(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


def same_table(a, b):
    a, b = np.ascontiguousarray(a, CLUSTER_DTYPE), np.ascontiguousarray(b, CLUSTER_DTYPE)
    return len(a) == len(b) and all(a[f].tobytes() == b[f].tobytes() for f in CLUSTER_DTYPE.names)


# ---- the four files, as text ----
def ps_head(r, x1, x2, fm, lx, ly):
    m = 10 * r[0]
    ps = "%!PS-Adobe-3.0 EPSF-3.0 \n"
    ps += "%%%%BoundingBox: %f %f %f %f \n" % (-m, -m, lx + m, ly + m)
    ps += "%%Creator: lbmdem-hip \n%%Title: DEM Grains & Forces \n0.1 setlinewidth 0.0 setgray \n"
    for i in range(len(r)):
        ps += "newpath %e %e %e 0.0 setlinewidth %.2f setgray 0 360 arc gsave fill grestore\n" % (
            x1[i] * 10000, x2[i] * 10000, r[i] * 10000, 0.8 - fm[i] / 2)
    return ps


def files_text(r, x1, x2, fm, rec, R, fmin, relative, zmin, t, lx, ly):
    """-> (clusters.dat, cluster_table.dat, _clusters.ps, the line of clusters.data) for a restatement R"""
    n = len(r)
    dat = "# fmin %e relative %d zmin %d threshold %e\n# i label degree core walls\n" % (fmin, 1 if relative else 0, zmin, R["thr"])
    dat += "".join("%d %d %d %d %d\n" % (i, R["label"][i], R["degree"][i], R["core"][i], R["walls"][i]) for i in range(n))
    tab = "".join("%d %d %d %d %d %e %e %e %e\n" % tuple(e[f] for f in CLUSTER_DTYPE.names) for e in R["table"])
    ps = ps_head(r, x1, x2, fm, lx, ly)
    for c in rec:
        if c["j"] >= 0 and c["fn"] >= R["thr"]:
            i, j = c["i"], c["j"]
            ps += "%e setlinewidth \n %s setrgbcolor \n" % (c["fn"], PALETTE[R["label"][i] % 8])
            ps += "1 setlinecap \n newpath \n"
            ps += "%e %e moveto \n %e %e lineto\n" % (x1[i] * 10000, x2[i] * 10000, x1[j] * 10000, x2[j] * 10000)
            ps += "stroke \n"
    line = "%e %e" % (t, R["thr"]) + "".join(" %d" % R["counts"][k] for k in COUNTERS) + "\n"
    return dat, tab, ps, line
