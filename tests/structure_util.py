"""The restatement of the packing structure analysis (lbmdem_structure_compute, include/lbmdem_hip.h) in numpy, all pairs and
serial: the neighbour list, the pair histogram from the table of squared edges, the bonds, and the bond-order and fabric sums as
per-grain Python loops in the stated order; and the three files' text by Python's `%`. IEEE double throughout: numpy's
elementwise operations and Python's float arithmetic round once per operation, as the contract asks."""
import math

import numpy as np

STRUCTURE_DTYPE = np.dtype([("nb", np.int32), ("bonds", np.int32), ("c6", np.float64), ("s6", np.float64), ("c2", np.float64),
                            ("s2", np.float64)])
COUNTERS = ("entries", "pairs", "bonded_pairs", "max_neighbours", "lone_grains", "six_bonds", "coincident_pairs",
            "nonfinite_grains")
DATA_HEADER = ("# t entries pairs bonded_pairs max_neighbours lone_grains six_bonds coincident_pairs nonfinite_grains psi6 "
               "fabric\n")
PI = 3.141592653589793


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def edges(rcut, nbins):
    """e2[nbins + 1]: (k*dr)*(k*dr) with dr = rcut / nbins, then rcut*rcut"""
    dr = np.float64(rcut) / np.float64(nbins)
    k = np.arange(nbins, dtype=np.float64)
    return np.concatenate([(k * dr) * (k * dr), [np.float64(rcut) * np.float64(rcut)]])


class Restatement:
    """all pairs of one set of centres, once; at(rcut, nbins, shell) restates a compute"""

    def __init__(self, x, y, r):
        self.x, self.y, self.r = (np.ascontiguousarray(a, np.float64) for a in (x, y, r))
        self.n = len(self.x)
        with np.errstate(all="ignore"):
            self.dx = self.x[None, :] - self.x[:, None]          # [i, j] = x_j - x_i
            self.dy = self.y[None, :] - self.y[:, None]
            self.d2 = self.dx * self.dx + self.dy * self.dy       # two products, then one addition
        self.rsum = self.r[:, None] + self.r[None, :]
        self.off_diagonal = ~np.eye(self.n, dtype=bool)

    def at(self, rcut, nbins, shell):
        n, d2 = self.n, self.d2
        rc2 = np.float64(rcut) * np.float64(rcut)
        with np.errstate(all="ignore"):
            nbr = (d2 <= rc2) & self.off_diagonal                 # (False with a NaN, False with an infinite centre)
            b = np.float64(shell) * self.rsum
            bonded = nbr & (d2 <= b * b)
        nb = nbr.sum(1).astype(np.int32)
        offsets = np.concatenate([[0], np.cumsum(nb)]).astype(np.int32)
        nbr_list = np.nonzero(nbr)[1].astype(np.int32)            # row-major: every grain's neighbours ascending
        e2 = edges(rcut, nbins)
        upper = np.triu(nbr, 1)
        d2_pairs = d2[upper]
        k = np.searchsorted(e2[:nbins], d2_pairs, side="right") - 1   # the last bin with e2[k] <= d2; the table alone decides
        hist = np.bincount(k, minlength=nbins).astype(np.int64)
        g = np.zeros(n, STRUCTURE_DTYPE)
        g["nb"], g["bonds"] = nb, bonded.sum(1)
        for i in range(n):
            c6 = s6 = c2 = s2 = 0.0
            for j in np.nonzero(bonded[i])[0]:                    # ascending
                q = float(d2[i, j])
                if not q > 0.0:
                    continue
                dx, dy = float(self.dx[i, j]), float(self.dy[i, j])
                d = math.sqrt(q)
                nx, ny = dx / d, dy / d
                a2, b2 = nx * nx - ny * ny, 2. * nx * ny
                a4, b4 = a2 * a2 - b2 * b2, 2. * a2 * b2
                a6, b6 = a4 * a2 - b4 * b2, b4 * a2 + a4 * b2
                c2 += a2; s2 += b2; c6 += a6; s6 += b6
            g["c6"][i], g["s6"][i], g["c2"][i], g["s2"][i] = c6, s6, c2, s2
        counts = dict(entries=int(nb.sum()), pairs=int(upper.sum()), bonded_pairs=int(np.triu(bonded, 1).sum()),
                      max_neighbours=int(nb.max()), lone_grains=int((nb == 0).sum()), six_bonds=int((g["bonds"] == 6).sum()),
                      coincident_pairs=int((upper & (d2 == 0)).sum()),
                      nonfinite_grains=int((~(np.isfinite(self.x) & np.isfinite(self.y))).sum()))
        return dict(offsets=offsets, nbr=nbr_list, hist=hist, grains=g, counts=counts, e2=e2)


def restate(x, y, r, rcut, nbins, shell):
    return Restatement(x, y, r).at(rcut, nbins, shell)


def order_parameters(g):
    """psi6 and fabric of structure.data: serial sums by index"""
    psi, C2, S2, withb, B = 0.0, 0.0, 0.0, 0, 0
    for row in g:
        C2 += float(row["c2"]); S2 += float(row["s2"])
        B += int(row["bonds"])
        if row["bonds"] > 0:
            c6, s6 = float(row["c6"]), float(row["s6"])
            psi += math.sqrt(c6 * c6 + s6 * s6) / float(int(row["bonds"]))
            withb += 1
    return (psi / float(withb) if withb else 0.0), (math.sqrt(C2 * C2 + S2 * S2) / float(B) if B else 0.0)


def files_text(g, rcut, nbins, shell, hist, counts, t, W, H):
    """-> (structure%.6i.dat, gr%.6i.dat, the line of structure.data)"""
    n = len(g)
    a = "# rcut %e nbins %d shell %e\n# i neighbours bonds c6 s6 c2 s2\n" % (rcut, nbins, shell)
    a += "".join("%d %d %d %e %e %e %e\n" % (i, row["nb"], row["bonds"], row["c6"], row["s6"], row["c2"], row["s2"])
                 for i, row in enumerate(g))
    e2 = edges(rcut, nbins)
    b = "# rcut %e nbins %d n %d W %e H %e\n" % (rcut, nbins, n, W, H)
    b += ("# k r_lo r_hi count g; g = count / (((n (n - 1) / 2 * pi) * (e2[k+1] - e2[k])) / (W * H)), 0 where that is no "
          "positive number; no edge correction\n")
    npairs_all = (float(n) * float(n - 1)) / 2.
    for k in range(nbins):
        ideal = ((npairs_all * PI) * (float(e2[k + 1]) - float(e2[k]))) / (float(W) * float(H))
        gk = float(int(hist[k])) / ideal if ideal > 0 else 0.0
        b += "%d %e %e %d %e\n" % (k, math.sqrt(float(e2[k])), math.sqrt(float(e2[k + 1])), hist[k], gk)
    psi6, fabric = order_parameters(g)
    c = "%e" % t + "".join(" %d" % counts[k] for k in COUNTERS) + " %e %e\n" % (psi6, fabric)
    return a, b, c
