"""The coarse-grained fields (include/lbmdem_hip.h: lbmdem_coarse_fields) restated in numpy, bit for bit.

Every number of a record is a chain of additions in a fixed order from +0.0. np.cumsum along an axis is a strict left-to-right
sum, so the last element of a cumsum over a block that begins with a column of +0.0 IS that chain; the grain block is a plain
loop over the grains in index order. The inputs are only what the handle's pinned downloads show -- f, obst, kinematics, fhf,
config(), walls(), grain_table() when the last sub-step was a table sub-step -- and the radii the handle was created with (m
and It follow from them, main.c:624-626)."""
import numpy as np

FIELDS = ("nodes fluid_nodes grain_nodes wall_nodes sum_rho sum_jx sum_jy sum_P grains sum_m sum_mv1 sum_mv2 sum_Iw "
          "ke_x ke_y ke_teta sum_fhf1 sum_fhf2 sum_fhf3 sum_z sum_p M11 M12 M21 M22").split()
DTYPE = np.dtype([(name, np.float64) for name in FIELDS])
NODE_BLOCK, GRAIN_BLOCK, CONTACT_BLOCK = FIELDS[:8], FIELDS[8:19], FIELDS[19:]
EX = (0, -1, -1, -1, 0, 1, 1, 1, 0)   # main.c:70-71
EY = (0, 1, 0, -1, -1, -1, 0, 1, 1)
RHO_S, REF_PI = 2650, 3.14159265358979   # main.c:42, 44


def grid(lx, ly, cw, ch):
    return (lx + cw - 1) // cw, (ly + ch - 1) // ch


def chain(block, axis):
    """per line along `axis`: +0.0 + b[0] + b[1] + ..., left to right"""
    zero = np.zeros_like(np.take(block, [0], axis=axis))
    return np.take(np.cumsum(np.concatenate([zero, block], axis=axis), axis=axis), -1, axis=axis)


def node_values(f, rho_moy):
    """rho, jx, jy (lbmdem_download_macro's values) and P of every node"""
    rho = np.zeros(f.shape[:2]); jx = np.zeros(f.shape[:2]); jy = np.zeros(f.shape[:2])
    for q in range(9):
        rho = rho + f[:, :, q]
        jx = jx + f[:, :, q] * EX[q]
        jy = jy + f[:, :, q] * EY[q]
    return rho, jx, jy, (1. / 3.) * rho_moy * (rho - 1.)


def node_block(out, f, obst, nbgrains, rho_moy, cw, ch):
    lx, ly = obst.shape
    ncx, ncy = out.shape
    fluid = obst == -1
    classes = {"fluid_nodes": fluid, "grain_nodes": (obst >= 0) & (obst < nbgrains), "wall_nodes": obst == nbgrains}
    values = dict(zip(("sum_rho", "sum_jx", "sum_jy", "sum_P"), node_values(f, rho_moy)))
    planes = {k: np.where(fluid, v, 0.0) for k, v in values.items()}
    planes.update({k: m.astype(np.float64) for k, m in classes.items()})
    for name, v in planes.items():
        col = np.zeros((lx, ncy))   # one sum per (x, cy): the chain over the cell's y
        for cy in range(ncy):
            col[:, cy] = chain(v[:, cy * ch:min(ly, (cy + 1) * ch)], 1)
        for cx in range(ncx):       # ... then over the cell's x
            out[name][cx, :] = chain(col[cx * cw:min(lx, (cx + 1) * cw), :], 0)
    out["nodes"] = out["fluid_nodes"] + out["grain_nodes"] + out["wall_nodes"]


def grain_block(out, r, kin, fhf, walls, dx, lx, ly, cw, ch, table=None):
    """-> grains outside. table: grain_table() when the last sub-step was a table sub-step, else None"""
    m = RHO_S * REF_PI * r * r
    It = m * r * r / 2
    Mgx, Mby = walls["Mgx"], walls["Mby"]
    outside = 0
    for i in range(len(r)):
        xc = (kin[i, 0] - Mgx) / dx
        yc = (kin[i, 1] - Mby) / dx
        if not (xc >= 0 and xc < lx and yc >= 0 and yc < ly):   # (false for NaN)
            outside += 1
            continue
        c = (int(xc) // cw, int(yc) // ch)
        v1, v2, v3 = kin[i, 3], kin[i, 4], kin[i, 5]
        add = {"grains": 1., "sum_m": m[i], "sum_mv1": m[i] * v1, "sum_mv2": m[i] * v2, "sum_Iw": It[i] * v3,
               "ke_x": 0.5 * m[i] * v1 * v1, "ke_y": 0.5 * m[i] * v2 * v2, "ke_teta": 0.5 * It[i] * v3 * v3,   # main.c:381-383
               "sum_fhf1": fhf[i, 0], "sum_fhf2": fhf[i, 1], "sum_fhf3": fhf[i, 2]}
        if table is not None:   # columns of main.c:182-197: p 13, M11..M22 21..24, z 28
            add.update({"sum_z": table[i, 28], "sum_p": table[i, 13], "M11": table[i, 21], "M12": table[i, 22],
                        "M21": table[i, 23], "M22": table[i, 24]})
        for name, v in add.items():
            out[name][c] = out[name][c] + v
    return outside


def expected(sim, r, cw, ch, table="ask"):
    """-> (cells, outside, contacts_valid) for the handle's present state. table "ask": grain_table() when the handle gives
    one; None: the last sub-step was no table sub-step; else the table itself"""
    cfg = sim.config()
    lx, ly = cfg.lx, cfg.ly
    if isinstance(table, str):
        try:
            table = sim.grain_table()
        except Exception:
            table = None
    out = np.zeros(grid(lx, ly, cw, ch), DTYPE)
    node_block(out, sim.f, sim.obst, cfg.nbgrains, cfg.phys.rho_moy, cw, ch)
    outside = grain_block(out, np.asarray(r, dtype=np.float64), sim.kinematics, sim.fhf, sim.walls(), cfg.dx, lx, ly, cw, ch, table)
    return out, outside, int(table is not None)


def mismatches(got, want):
    """members that are not array_equal (NaN never equals: a NaN anywhere is a finding)"""
    return [name for name in FIELDS if not np.array_equal(got[name], want[name])]


def file_text(cw, ch, cells, outside, contacts_valid):
    """coarse%.6i.dat as the header documents it"""
    ncx, ncy = cells.shape
    text = "# cw %d ch %d ncx %d ncy %d outside %d contacts %d\n" % (cw, ch, ncx, ncy, outside, contacts_valid)
    for cx in range(ncx):
        for cy in range(ncy):
            text += "%d %d" % (cx, cy) + "".join(" %e" % cells[name][cx, cy] for name in FIELDS) + "\n"
    return text
