"""The strain analysis restated in numpy (include/lbmdem_hip.h, "Strain fields"): the mark is a set of centres, angles and a CSR
neighbour list; the compute compares the grains where they are now with it. The chains go neighbour rank by neighbour rank over the
CSR -- rank 0 of every grain, then rank 1, ... -- so every grain's sums are added in list order, one IEEE double operation per numpy
call (no contraction): the association is the stated one and the device is compared on the bits. Also the formatter's derived
columns and the sums of strain.data, and the fixed-radius list the structure analysis would make (all pairs)."""
import numpy as np

STRAIN_DTYPE = np.dtype([("ux", np.float64), ("uy", np.float64), ("drot", np.float64), ("Fxx", np.float64), ("Fxy", np.float64),
                         ("Fyx", np.float64), ("Fyy", np.float64), ("d2min", np.float64), ("used", np.int32), ("lost", np.int32),
                         ("flags", np.int32)])
COUNTERS = ("fitted", "few", "degenerate", "nonfinite_grains", "entries", "used", "lost", "worst_grain")
DOUBLES = STRAIN_DTYPE.names[:8]
INTS = STRAIN_DTYPE.names[8:]
NONFINITE, FEW, DEGENERATE = 1, 2, 4
DATA_HEADER = "# t fitted few degenerate nonfinite_grains entries used lost worst_grain msd mean_d2min max_d2min\n"
TINY = 2.0 ** -40


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def neighbour_list(x, y, rcut):
    """-> (offsets int32 [n + 1], nbr int32 [entries], rc2): j is a neighbour of i iff j != i and d2 <= rcut*rcut, ascending"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    rc2 = np.float64(rcut) * np.float64(rcut)
    with np.errstate(all="ignore"):
        dx, dy = x[None, :] - x[:, None], y[None, :] - y[:, None]
        near = (dx * dx + dy * dy) <= rc2
    np.fill_diagonal(near, False)
    off = np.zeros(len(x) + 1, np.int32)
    off[1:] = np.cumsum(near.sum(axis=1))
    return off, np.nonzero(near)[1].astype(np.int32), float(rc2)


def key_of(d2min):
    """the order of the argmax: the bits of a double >= +0.0 as an unsigned integer, 0 for anything else"""
    d = np.ascontiguousarray(d2min, np.float64)
    with np.errstate(all="ignore"):
        return np.where(d >= 0.0, d.view(np.uint64), np.uint64(0))


def restate(X0, Y0, T0, off, nbr, rc2, x, y, th):
    """one compute -> dict(grains: [n] of STRAIN_DTYPE, counts: dict of COUNTERS)"""
    X0, Y0, T0, x, y, th = (np.ascontiguousarray(a, np.float64) for a in (X0, Y0, T0, x, y, th))
    off, nbr = np.asarray(off, np.int64), np.asarray(nbr, np.int64)
    n = len(x)
    deg = off[1:] - off[:-1]
    g = np.zeros(n, STRAIN_DTYPE)
    fin = np.isfinite(x) & np.isfinite(y) & np.isfinite(X0) & np.isfinite(Y0)
    used, lost = np.zeros(n, np.int64), np.zeros(n, np.int64)
    S = {k: np.zeros(n) for k in ("Xxx", "Xxy", "Xyx", "Xyy", "Yxx", "Yxy", "Yyy")}
    F = {k: np.zeros(n) for k in ("Fxx", "Fxy", "Fyx", "Fyy")}
    d2 = np.zeros(n)

    def rank_of(who, rank):
        """the grains of `who` that have a neighbour of this rank which is not skipped, and d0x, d0y, dx, dy to it"""
        I = np.nonzero(who & (deg > rank))[0]
        J = nbr[off[I] + rank]
        d0x, d0y, dx, dy = X0[J] - X0[I], Y0[J] - Y0[I], x[J] - x[I], y[J] - y[I]
        ok = np.isfinite(dx) & np.isfinite(dy)
        return I[ok], d0x[ok], d0y[ok], dx[ok], dy[ok]

    with np.errstate(all="ignore"):
        for rank in range(int(deg.max()) if n else 0):
            I, d0x, d0y, dx, dy = rank_of(fin, rank)
            used[I] += 1
            lost[I] += (dx * dx + dy * dy) > rc2
            S["Xxx"][I] += dx * d0x; S["Xxy"][I] += dx * d0y; S["Xyx"][I] += dy * d0x; S["Xyy"][I] += dy * d0y
            S["Yxx"][I] += d0x * d0x; S["Yxy"][I] += d0x * d0y; S["Yyy"][I] += d0y * d0y
        det = S["Yxx"] * S["Yyy"] - S["Yxy"] * S["Yxy"]
        few = fin & (used < 2)
        degenerate = fin & ~few & ~(det > TINY * (S["Yxx"] * S["Yyy"]))
        fit = fin & ~few & ~degenerate
        I = np.nonzero(fit)[0]
        Ixx, Ixy, Iyy = S["Yyy"][I] / det[I], (-S["Yxy"][I]) / det[I], S["Yxx"][I] / det[I]
        F["Fxx"][I] = S["Xxx"][I] * Ixx + S["Xxy"][I] * Ixy
        F["Fxy"][I] = S["Xxx"][I] * Ixy + S["Xxy"][I] * Iyy
        F["Fyx"][I] = S["Xyx"][I] * Ixx + S["Xyy"][I] * Ixy
        F["Fyy"][I] = S["Xyx"][I] * Ixy + S["Xyy"][I] * Iyy
        for rank in range(int(deg[fit].max()) if fit.any() else 0):
            I, d0x, d0y, dx, dy = rank_of(fit, rank)
            rx = dx - (F["Fxx"][I] * d0x + F["Fxy"][I] * d0y)
            ry = dy - (F["Fyx"][I] * d0x + F["Fyy"][I] * d0y)
            d2[I] += rx * rx + ry * ry
        g["ux"][fin], g["uy"][fin], g["drot"][fin] = (x - X0)[fin], (y - Y0)[fin], (th - T0)[fin]
    for k in F:
        g[k] = F[k]
    g["d2min"] = d2
    g["used"], g["lost"] = used, lost
    g["flags"] = np.where(~fin, NONFINITE, 0) | np.where(few, FEW, 0) | np.where(degenerate, DEGENERATE, 0)
    worst = -1
    if fit.any():
        I = np.nonzero(fit)[0]
        worst = int(I[np.argmax(key_of(d2[I]))])          # (argmax: the first among equals)
    counts = dict(zip(COUNTERS, (int(fit.sum()), int(few.sum()), int(degenerate.sum()), int((~fin).sum()), int(deg.sum()),
                                 int(used.sum()), int(lost.sum()), worst)))
    return dict(grains=g, counts=counts)


def derived(g):
    """the six derived columns of strain%.6i.dat -> dict of [n] doubles; zeros where the grain is not fitted"""
    fit = g["flags"] == 0
    z = lambda a: np.where(fit, a, 0.0)
    with np.errstate(all="ignore"):
        exx, eyy = z(g["Fxx"] - 1.0), z(g["Fyy"] - 1.0)
        exy, omega = z(0.5 * (g["Fxy"] + g["Fyx"])), z(0.5 * (g["Fyx"] - g["Fxy"]))
        vol = exx + eyy
        h = 0.5 * (exx - eyy)
        dev = np.sqrt(h * h + exy * exy)
    return dict(exx=exx, eyy=eyy, exy=exy, omega=omega, vol=vol, dev=dev)


def data_sums(g):
    """msd, the mean d2min/used and the largest d2min of strain.data: serial sums by index"""
    su2, sd2, big, moved, fitted = 0.0, 0.0, 0.0, 0, 0
    for row in g:
        ux, uy, d2m = float(row["ux"]), float(row["uy"]), float(row["d2min"])
        if not row["flags"] & NONFINITE:
            su2 += ux * ux + uy * uy
            moved += 1
        if row["flags"] == 0:
            sd2 += d2m / float(row["used"])
            fitted += 1
            if d2m > big:
                big = d2m
    return (su2 / moved if moved else 0.0), (sd2 / fitted if fitted else 0.0), big


def files_text(g, rc2, counts, t, t_mark):
    """-> (strain%.6i.dat, the line of strain.data)"""
    D = derived(g)
    a = "# rc2 %e t_mark %e\n# i ux uy drot exx eyy exy omega vol dev d2min used lost flags\n" % (rc2, t_mark)
    a += "".join("%d %e %e %e %e %e %e %e %e %e %e %d %d %d\n" % (
        i, row["ux"], row["uy"], row["drot"], D["exx"][i], D["eyy"][i], D["exy"][i], D["omega"][i], D["vol"][i], D["dev"][i],
        row["d2min"], row["used"], row["lost"], row["flags"]) for i, row in enumerate(g))
    msd, md2, big = data_sums(g)
    b = "%e" % t + "".join(" %d" % counts[k] for k in COUNTERS) + " %e %e %e\n" % (msd, md2, big)
    return a, b
