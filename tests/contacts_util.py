"""Shared by the contact network tests (tests/test_contacts_host.py, tests/test_contacts_golden_regen.py,
tests/test_gpu_contacts.py) and the generator of their golden files (tests/golden/make_contacts_golden.py).

A numpy restatement of what a sub-step does to a contact, in plain float64 elementwise arithmetic (no FMA, np.sqrt is the
correctly rounded square root): the drift and half kick (main.c:1748-1753), the two grain-grain laws (force_grains,
main.c:739-774; the inline film law, main.c:1365-1395) and the four wall laws (force_WallB/T/L/R, main.c:809-951); and
`replay`, which adds a record list into the per-grain sums the reference accumulates (main.c:776-799, 1397-1416, 830-838,
875-882, 907-915, 938-949). Expressions are written with the reference's operand order: the comparisons are on the bits."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
WALL_B, WALL_T, WALL_L, WALL_R = -1, -2, -3, -4
CONTACT_DTYPE = np.dtype([("i", np.int32), ("j", np.int32), ("dn", np.float64), ("nx", np.float64), ("ny", np.float64),
                          ("fn", np.float64), ("ft", np.float64)])
COUNTERS = ("candidate_pairs", "touching_pairs", "coulomb_clamped", "fn_zero", "wall_contacts", "grains_in_contact")
# the columns of the 30-column grain table (main.c:182-197) that a record list decides
TABLE_COLS = dict(p=13, s=14, f1=15, f2=16, ifm=17, M11=21, M12=22, M21=23, M22=24, z=28, zz=29)
# the initialised globals of main.c:97-118, 163-165 that the laws read
PHYSICS = dict(km=3e+6, kg=1.6e+6, kt=1.0e+6, ktm=2e+6, nug=6.4e+1, num=8.7e+1, nugt=5e-1, mu=.5317, mum=.466, mumb=.466,
               murf=0.01, freq=5., amp=4.e-4, stepFilm=8000)
CASES = ("contacts_Ca_64x48", "contacts_Cb_256x200", "contacts_Cfilm_256x200")


def params(dt, dt2, Mgx, Mdx, Mby, Mhy, t=0.0, **over):
    """what the laws read: the reference's globals plus the scalars of a run (main.c:855: the top wall's velocity)"""
    P = dict(PHYSICS)
    P.update(over)
    P.update(dt=float(dt), dt2=float(dt2), Mgx=float(Mgx), Mdx=float(Mdx), Mby=float(Mby), Mhy=float(Mhy))
    P["wallT_vel"] = P["amp"] * P["freq"] * np.cos(P["freq"] * float(t))
    return P


def params_of_config(cfg, wallT_vel=None):
    """the same from a lbmdem_config as the sub-step found it"""
    ph = cfg.phys
    P = params(cfg.dt, cfg.dt2, cfg.Mgx, cfg.Mdx, cfg.Mby, cfg.Mhy, t=ph.t,
               **{k: float(getattr(ph, k)) for k in "km kg kt ktm nug num nugt mu mum mumb murf freq amp".split()})
    if wallT_vel is not None:
        P["wallT_vel"] = float(wallT_vel)
    return P


def advance(k9, P):
    """drifted + half-kicked x1, x2, v1, v2, v3 of every grain from the 9 kinematic columns (main.c:1748-1753)"""
    k9 = np.asarray(k9, np.float64)
    dt, dt2 = P["dt"], P["dt2"]
    x1 = k9[:, 0] + dt * k9[:, 3] + dt2 * k9[:, 6] / 2.
    x2 = k9[:, 1] + dt * k9[:, 4] + dt2 * k9[:, 7] / 2.
    v1 = k9[:, 3] + dt * k9[:, 6] / 2.
    v2 = k9[:, 4] + dt * k9[:, 7] / 2.
    v3 = k9[:, 5] + dt * k9[:, 8] / 2.
    return x1, x2, v1, v2, v3


def pairs_of_list(cumul, neigh):
    """(m, 2) candidate pairs i < j in the reference's loop order from its cumul / neighbours arrays"""
    cumul = np.asarray(cumul, np.int64).copy()
    cumul[-1] = cumul[-2] if len(cumul) > 1 else 0   # (initVerlet never writes the last grain's entry: it has no higher partner)
    counts = np.diff(np.concatenate([[0], cumul]))
    i = np.repeat(np.arange(len(cumul)), counts)
    return np.stack([i, np.asarray(neigh, np.int64)[:len(i)]], axis=1)


def wallflags_of_lists(n, lists):
    """bit 0..3 = candidate of the bottom, top, left, right wall, from the reference's four wall lists"""
    wf = np.zeros(n, np.int32)
    for bit, l in enumerate(lists):
        wf[np.asarray(l, np.int64)] |= 1 << bit
    return wf


def pair_records(S, r, pairs, P, film):
    """the grain-grain records of the candidates `pairs` in their order, and which of them took the Coulomb clamp branch"""
    x1, x2, v1, v2, v3 = S
    i, j = pairs[:, 0], pairs[:, 1]
    xij = x1[i] - x1[j]
    yij = x2[i] - x2[j]
    dist = np.sqrt(xij * xij + yij * yij)
    dn = dist - r[i] - r[j]
    t = ~(dn >= 0)
    i, j, xij, yij, dist, dn = i[t], j[t], xij[t], yij[t], dist[t], dn[t]
    vx = v1[i] - v1[j]
    vy = v2[i] - v2[j]
    xn = xij / dist
    yn = yij / dist
    vn = vx * xn + vy * yn
    vt = -vx * yn + vy * xn - v3[i] * r[i] - v3[j] * r[j]
    fn = -P["kg"] * dn - P["nug"] * vn
    fn = np.where(fn < 0, 0.0, fn)
    if not film:       # main.c:761-771
        ft = -P["kt"] * vt * P["dt"]
        ftest = P["mu"] * fn
        clamp = np.abs(ft) > ftest
        ft = np.where(clamp, np.where(ft < 0.0, ftest, -ftest), ft)
    else:              # main.c:1382-1391
        ft = P["kt"] * vt * P["dt"]
        ftest = P["mu"] * ft
        clamp = np.abs(ft) > ftest
        ft = np.where(clamp, np.where(ft > 0.0, ftest, -ftest), ft)
    rec = np.zeros(len(i), CONTACT_DTYPE)
    rec["i"], rec["j"], rec["dn"], rec["nx"], rec["ny"], rec["fn"], rec["ft"] = i, j, dn, xn, yn, fn, ft
    return rec, clamp


def wall_records(S, r, wf, P):
    """the wall records: grain ascending, bottom, top, left, right within a grain"""
    x1, x2, v1, v2, v3 = S
    n = len(r)
    g = np.arange(n)
    out = []
    # force_WallB, main.c:809-828
    dn = x2 - r - P["Mby"]
    m = ((wf & 1) != 0) & (dn < 0)
    fn = -P["km"] * dn - P["num"] * v2
    fn = np.where(fn < 0, 0., fn)
    ft = P["ktm"] * v1
    ftest = P["mumb"] * fn
    ft = np.where(np.abs(ft) > ftest, np.where(ft < 0.0, ftest, -ftest), ft)
    out.append((g[m], WALL_B, dn[m], 0., 1., fn[m], ft[m]))
    # force_WallT, main.c:846-871
    dn = -x2 - r + P["Mhy"]
    m = ((wf & 2) != 0) & (dn < 0)
    fn = P["km"] * dn - P["num"] * v2
    fn = np.where(fn > 0., 0., fn)
    vt = v1 + v3 * r - P["wallT_vel"]
    ft = np.abs(P["ktm"] * vt)
    ftmax = np.where(vt >= 0, P["mumb"] * fn - P["nugt"] * vt, P["mumb"] * fn + P["nugt"] * vt)
    ft = np.where(ft > ftmax, ftmax, ft)
    ft = np.where(vt > 0, -ft, ft)
    out.append((g[m], WALL_T, dn[m], 0., -1., fn[m], ft[m]))
    # force_WallL, main.c:888-904
    dn = x1 - r - P["Mgx"]
    m = ((wf & 4) != 0) & (dn < 0)
    fn = -P["km"] * dn + P["num"] * v1
    fn = np.where(fn < 0., 0., fn)
    ft = P["mum"] * fn
    ft = np.where(v2 > 0, -ft, ft)
    out.append((g[m], WALL_L, dn[m], 1., 0., fn[m], ft[m]))
    # force_WallR, main.c:923-936: ft from the unclamped fn
    dn = -x1 - r + P["Mdx"]
    m = ((wf & 8) != 0) & (dn < 0)
    fn = P["km"] * dn - P["num"] * v1
    ft = P["mum"] * fn
    ft = np.where(v2 > 0, -ft, ft)
    fn = np.where(fn > 0., 0., fn)
    out.append((g[m], WALL_R, dn[m], -1., 0., fn[m], ft[m]))
    rec = np.zeros(sum(len(o[0]) for o in out), CONTACT_DTYPE)
    at = 0
    for gi, code, dn, nx, ny, fn, ft in out:
        s = slice(at, at + len(gi))
        rec["i"][s], rec["j"][s], rec["dn"][s], rec["nx"][s], rec["ny"][s], rec["fn"][s], rec["ft"][s] = gi, code, dn, nx, ny, fn, ft
        at += len(gi)
    return rec[np.lexsort((-rec["j"], rec["i"]))]   # grain ascending, then B, T, L, R (codes -1 .. -4)


def restate(k9, r, pairs, wf, P, film):
    """-> (records in the export's order, the six counters of lbmdem_contact_stats) for a sub-step that starts from `k9`"""
    r = np.asarray(r, np.float64)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    S = advance(k9, P)
    pr, clamp = pair_records(S, r, pairs, P, film)
    wr = wall_records(S, r, np.asarray(wf), P)
    rec = np.concatenate([pr, wr])
    grains = set(pr["i"].tolist()) | set(pr["j"].tolist()) | set(wr["i"].tolist())
    counts = dict(zip(COUNTERS, (len(pairs), len(pr), int(clamp.sum()), int((pr["fn"] == 0).sum()), len(wr), len(grains))))
    return rec, counts


def replay(records, x1, x2, n, film, dt, mu):
    """per-grain p, s, f1, f2, ifm, M11, M12, M21, M22 (float64) and z, zz (int) from a record list, added in record order.
    x1, x2: the positions the sub-step evaluated its contacts at (the drifted ones: what the table holds afterwards)."""
    out = {k: np.zeros(n) for k in "p s f1 f2 ifm M11 M12 M21 M22".split()}
    out["z"] = np.zeros(n, np.int64)
    out["zz"] = np.zeros(n, np.int64)
    adt = abs(dt)
    for c in records:
        i, j, fn, ft = int(c["i"]), int(c["j"]), float(c["fn"]), float(c["ft"])
        if j >= 0:
            f1 = fn * c["nx"] - ft * c["ny"]
            f2 = fn * c["ny"] + ft * c["nx"]
            xij, yij = x1[i] - x1[j], x2[i] - x2[j]
            out["p"][i] += fn; out["p"][j] += fn
            out["s"][i] += ft; out["s"][j] += ft
            out["z"][i] += 1
            if not film:   # main.c:776-799
                out["f1"][i] += f1; out["f2"][i] += f2
                out["zz"][i] += 1
                if fn == 0:
                    out["ifm"][i] = 0
                else:
                    out["ifm"][i] += abs(ft / (mu * fn))
            out["M11"][i] += f1 * xij; out["M12"][i] += f1 * yij
            out["M21"][i] += f2 * xij; out["M22"][i] += f2 * yij
        elif j == WALL_B:   # f1 = ft, f2 = fn; main.c:830-838
            out["p"][i] += fn; out["s"][i] += ft; out["f1"][i] += ft; out["z"][i] += 1
            out["M12"][i] += ft * dt; out["M22"][i] += fn * dt
        elif j == WALL_T:   # f1 = ft, f2 = fn; main.c:875-882
            out["M12"][i] += ft * adt; out["M22"][i] += fn * adt
            out["p"][i] += fn; out["s"][i] += ft; out["z"][i] += 1
        elif j == WALL_L:   # f1 = fn, f2 = ft; main.c:907-915
            out["M11"][i] += fn * adt; out["M21"][i] += ft * adt
            out["p"][i] += fn; out["s"][i] += ft; out["f1"][i] += fn; out["z"][i] += 1
        elif j == WALL_R:   # f1 = fn, f2 = -ft; main.c:938-949
            out["p"][i] += fn; out["f1"][i] += fn
            out["M11"][i] += fn * adt; out["M21"][i] += (-ft) * adt
            out["z"][i] += 1
        else:
            raise ValueError(f"unknown wall code {j}")
    return out


def table_mismatches(rep, table):
    """the columns of `table` (30 per grain) whose bits differ from a replay's"""
    table = np.asarray(table, np.float64)
    return [name for name, col in TABLE_COLS.items()
            if rep[name].astype(np.float64).tobytes() != np.ascontiguousarray(table[:, col]).tobytes()]


def same_records(a, b):
    """field by field, bit for bit, in the same order"""
    a, b = np.ascontiguousarray(a, CONTACT_DTYPE), np.ascontiguousarray(b, CONTACT_DTYPE)
    return len(a) == len(b) and all(a[f].tobytes() == b[f].tobytes() for f in CONTACT_DTYPE.names)


def load_case(name):
    return dict(np.load(os.path.join(HERE, "golden", name + ".npz")))


def case_params(g):
    """the parameters of a golden case's sub-step, from the scalars the generator stored"""
    s = g["scalars"]   # dx dtLB dt dt2 c npDEM Mgx Mdx Mby Mhy xG yG
    return params(s[2], s[3], s[6], s[7], s[8], s[9])


def case_film(g):
    return int(g["nbsteps"]) % PHYSICS["stepFilm"] == 0
