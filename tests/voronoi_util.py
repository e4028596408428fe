"""The restatement of the Voronoi analysis (lbmdem_voronoi_compute, include/lbmdem_hip.h): all pairs for the neighbour set, then
per grain the box clipped by every neighbour's radical line in ascending order and the measures of what is left, serially and in
the stated order; and the two files' text by Python's `%`. IEEE double throughout: numpy's elementwise operations and Python's
float arithmetic round once per operation, as the contract asks. numpy is used for one thing beyond the neighbour set: the s of
every vertex against every remaining neighbour at once (the same three operations per value), to find the next neighbour whose line
cuts something -- a line that cuts nothing leaves the polygon as it was."""
import math

import numpy as np

VORONOI_DTYPE = np.dtype([("area", np.float64), ("perimeter", np.float64), ("phi", np.float64), ("R2", np.float64),
                          ("faces", np.int32), ("walls", np.int32), ("nverts", np.int32), ("flags", np.int32)])
COUNTERS = ("cells", "complete", "empty", "overflowed", "nonfinite_grains", "grain_faces", "wall_faces", "max_faces")
DATA_HEADER = ("# t cells complete empty overflowed nonfinite_grains grain_faces wall_faces max_faces sum_area box_area mean_phi "
               "mean_faces\n")
PI = 3.141592653589793
MAXV = 32
COMPLETE, EMPTY, OVERFLOW, NONFINITE = 1, 2, 4, 8


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def clip(P, s, j):
    """one walk over the edges a -> b of P, s the vertices' values against j's line -> the new polygon"""
    Q, m = [], len(P)
    for k in range(m):
        a, b, sa, sb = P[k], P[(k + 1) % m], s[k], s[(k + 1) % m]
        ina, inb = sa <= 0.0, sb <= 0.0
        if ina:
            Q.append(a)
        if ina != inb:
            t = sa / (sa - sb)
            Q.append((a[0] + t * (b[0] - a[0]), a[1] + t * (b[1] - a[1]), j if ina else a[2]))
    return Q


def cell(xi, yi, ri, js, xj, yj, rj, box):
    """-> (polygon as a list of (vx, vy, src), overflowed); js ascending, xj, yj, rj theirs"""
    gx, dx_, by, hy = (float(v) for v in box)
    if not (math.isfinite(xi) and math.isfinite(yi)):
        return [], False
    P = [(gx, by, -1), (dx_, by, -2), (dx_, hy, -3), (gx, hy, -4)]
    with np.errstate(all="ignore"):
        dx, dy = xj - xi, yj - yi
        d2 = dx * dx + dy * dy
        h = 0.5 * ((d2 + ri * ri) - rj * rj)
        start = 0
        while P and start < len(js):
            ax = np.array([p[0] for p in P]) - xi
            ay = np.array([p[1] for p in P]) - yi
            s = (ax[None, :] * dx[start:, None] + ay[None, :] * dy[start:, None]) - h[start:, None]
            cuts = (d2[start:] > 0) & ~(s <= 0).all(1)
            if not cuts.any():
                break
            k = int(np.argmax(cuts))
            P = clip(P, [float(v) for v in s[k]], int(js[start + k]))
            if len(P) > MAXV:
                return [], True
            start += k + 1
    return P, False


def measures(P, xi, yi):
    """-> area, perimeter, R2, faces, walls, [(src, len) per face]"""
    A2 = per = R2 = 0.0
    faces = walls = 0
    rows, m = [], len(P)
    for k in range(m):
        a, b = P[k], P[(k + 1) % m]
        ax, ay, bx, by = a[0] - xi, a[1] - yi, b[0] - xi, b[1] - yi
        A2 += ax * by - bx * ay
        ex, ey = b[0] - a[0], b[1] - a[1]
        length = math.sqrt(ex * ex + ey * ey)
        per += length
        q = ax * ax + ay * ay
        if q > R2:
            R2 = q
        if a[0] != b[0] or a[1] != b[1]:
            rows.append((a[2], length))
            if a[2] >= 0:
                faces += 1
            else:
                walls |= 1 << (-a[2] - 1)
    return 0.5 * A2, per, R2, faces, walls, rows


class Restatement:
    """all pairs of one set of centres, once; at(rcut) restates a structure compute with that cutoff and the Voronoi compute"""

    def __init__(self, x, y, r, box):
        self.x, self.y, self.r = (np.ascontiguousarray(a, np.float64) for a in (x, y, r))
        self.box = tuple(float(v) for v in box)          # Mgx, Mdx, Mby, Mhy
        self.n = len(self.x)
        with np.errstate(all="ignore"):
            dx = self.x[None, :] - self.x[:, None]
            dy = self.y[None, :] - self.y[:, None]
            self.d2 = dx * dx + dy * dy
        self.off_diagonal = ~np.eye(self.n, dtype=bool)
        self.rmax = float(self.r.max())
        self.cache = {}

    def at(self, rcut):
        if rcut not in self.cache:
            self.cache[rcut] = self.make(rcut)
        return self.cache[rcut]

    def make(self, rcut):
        n, rcut = self.n, float(rcut)
        with np.errstate(all="ignore"):
            nbr = (self.d2 <= np.float64(rcut) * np.float64(rcut)) & self.off_diagonal
        g = np.zeros(n, VORONOI_DTYPE)
        foff, fsrc, flen, polys = [0], [], [], []
        for i in range(n):
            xi, yi, ri = float(self.x[i]), float(self.y[i]), float(self.r[i])
            js = np.nonzero(nbr[i])[0]
            P, over = cell(xi, yi, ri, js, self.x[js], self.y[js], self.r[js], self.box)
            area, per, R2, faces, walls, rows = measures(P, xi, yi)
            flags = 0
            if over:
                flags |= OVERFLOW
            elif not P:
                flags |= EMPTY
            if not (math.isfinite(xi) and math.isfinite(yi)):
                flags |= NONFINITE
            bound = 0.5 * (rcut + (ri * ri - self.rmax * self.rmax) / rcut)
            if len(P) > 0 and bound > 0 and R2 <= bound * bound:
                flags |= COMPLETE
            phi = ((PI * ri) * ri) / area if area > 0 else 0.0
            g[i] = (area, per, phi, R2, faces, walls, len(P), flags)
            fsrc += [s for s, _ in rows]
            flen += [l for _, l in rows]
            foff.append(len(fsrc))
            polys.append(P)
        nf = np.diff(foff)
        counts = dict(cells=int((g["area"] > 0).sum()), complete=int((g["flags"] & COMPLETE > 0).sum()),
                      empty=int((g["flags"] & EMPTY > 0).sum()), overflowed=int((g["flags"] & OVERFLOW > 0).sum()),
                      nonfinite_grains=int((g["flags"] & NONFINITE > 0).sum()), grain_faces=int(g["faces"].sum()),
                      wall_faces=int((nf - g["faces"]).sum()), max_faces=int(g["faces"].max()))
        return dict(grains=g, foff=np.array(foff, np.int32), fsrc=np.array(fsrc, np.int32), flen=np.array(flen, np.float64),
                    counts=counts, polys=polys)


def restate(x, y, r, box, rcut):
    return Restatement(x, y, r, box).at(rcut)


def data_means(g):
    """sum of area, mean phi and mean faces of voronoi.data: serial sums by index"""
    sa = sp = sf = 0.0
    k = 0
    for row in g:
        sa += float(row["area"])
        if row["flags"] & COMPLETE and row["area"] > 0:
            sp += float(row["phi"]); sf += float(int(row["faces"])); k += 1
    return sa, (sp / float(k) if k else 0.0), (sf / float(k) if k else 0.0)


def files_text(g, rcut, counts, t, W, H):
    """-> (voronoi%.6i.dat, the line of voronoi.data)"""
    a = "# rcut %e\n# i area perimeter phi faces walls nverts flags\n" % rcut
    a += "".join("%d %e %e %e %d %d %d %d\n" % (i, row["area"], row["perimeter"], row["phi"], row["faces"], row["walls"],
                                                 row["nverts"], row["flags"]) for i, row in enumerate(g))
    sa, mp, mf = data_means(g)
    b = "%e" % t + "".join(" %d" % counts[k] for k in COUNTERS) + " %e %e %e %e\n" % (sa, float(W) * float(H), mp, mf)
    return a, b
