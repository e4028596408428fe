"""The flow fields (include/lbmdem_hip.h: lbmdem_flow_fields, lbmdem_flow_sums) restated in numpy, bit for bit.

Elementwise numpy operations on float64 are IEEE operations, one rounding each, so an expression written with the header's
association IS the header's value. np.cumsum along an axis is a strict left-to-right sum, so the last element of a cumsum over a
block that begins with +0.0 is the chain the header asks for. The inputs are only what the handle's downloads show: f, obst,
kinematics, walls(), config()."""
import struct

import numpy as np

NAMES = ("ux", "uy", "vort", "div", "nxx", "nxy", "gdot", "diss")
SUMS = ("n_fluid", "sum_rho", "sum_ke", "sum_diss", "sum_enstrophy", "max_u2", "max_gdot", "max_abs_div")
ALL = 255
BLOCK = 64
DATA_HEADER = "# t n_fluid sum_rho sum_ke sum_diss sum_enstrophy max_u2 max_gdot max_abs_div\n"


def plane_names(mask):
    return [name for k, name in enumerate(NAMES) if mask >> k & 1]


def fields(f, obst, kin, Mgx, Mby, dx, c, s8, s9, nbgrains):
    """-> dict of the eight planes plus rho and the fluid mask"""
    lx, ly = obst.shape
    fluid = obst == -1
    grain = (obst >= 0) & (obst < nbgrains)
    q = [f[:, :, k] for k in range(9)]
    with np.errstate(all="ignore"):
        rho = q[0] + q[1] + q[2] + q[3] + q[4] + q[5] + q[6] + q[7] + q[8]   # main.c:1082
        jx = q[5] + q[6] + q[7] - q[1] - q[2] - q[3]                         # main.c:1091
        jy = q[1] + q[8] + q[7] - q[3] - q[4] - q[5]                         # main.c:1093
        pxx = q[2] - q[4] + q[6] - q[8]                                      # main.c:1095
        pxy = -q[1] + q[3] - q[5] + q[7]                                     # main.c:1096
        nxx = pxx - (jx * jx - jy * jy) / rho                                # main.c:1105
        nxy = pxy - jx * jy / rho                                            # main.c:1106
        D = -1.5 * s8 * nxx / rho
        T = -3. * s9 * nxy / rho
        nu8 = (1. / s8 - 0.5) / 3.
        nu9 = (1. / s9 - 0.5) / 3.
        gdot = np.sqrt(D * D + T * T)
        diss = rho * (nu8 * D * D + nu9 * T * T)
        ux_f = jx / rho
        uy_f = jy / rho
    # the grains' rigid-body velocity at their nodes: main.c:974-975 over c
    i = np.where(grain, obst, 0)
    x = np.arange(lx, dtype=np.float64)[:, None] * np.ones((1, ly))
    y = np.ones((lx, 1)) * np.arange(ly, dtype=np.float64)[None, :]
    x1, x2, v1, v2, v3 = (kin[:, k][i] for k in (0, 1, 3, 4, 5))
    ux_g = (v1 - (y * dx + Mby - x2) * v3) / c
    uy_g = (v2 + (x * dx + Mgx - x1) * v3) / c
    ux = np.where(fluid, ux_f, np.where(grain, ux_g, 0.0))
    uy = np.where(fluid, uy_f, np.where(grain, uy_g, 0.0))
    vort = np.zeros((lx, ly))
    div = np.zeros((lx, ly))
    vort[1:-1, 1:-1] = (uy[2:, 1:-1] - uy[:-2, 1:-1]) * 0.5 - (ux[1:-1, 2:] - ux[1:-1, :-2]) * 0.5
    div[1:-1, 1:-1] = (ux[2:, 1:-1] - ux[:-2, 1:-1]) * 0.5 + (uy[1:-1, 2:] - uy[1:-1, :-2]) * 0.5
    z = lambda a: np.where(fluid, a, 0.0)
    return dict(ux=ux, uy=uy, vort=vort, div=div, nxx=z(nxx), nxy=z(nxy), gdot=z(gdot), diss=z(diss), rho=z(rho), fluid=fluid,
                D=z(D), T=z(T))


def chain(block, axis):
    """per line along `axis`: +0.0 + b[0] + b[1] + ..., left to right"""
    zero = np.zeros_like(np.take(block, [0], axis=axis))
    return np.take(np.cumsum(np.concatenate([zero, block], axis=axis), axis=axis), -1, axis=axis)


def total(v):
    """the three-level chain: per row and block of 64 y, per row over its blocks, over the rows"""
    lx, ly = v.shape
    nb = (ly + BLOCK - 1) // BLOCK
    blocks = np.zeros((lx, nb))
    for b in range(nb):
        blocks[:, b] = chain(v[:, b * BLOCK:min(ly, (b + 1) * BLOCK)], 1)
    return float(chain(chain(blocks, 1)[None, :], 1)[0])


def sums(F):
    fl = F["fluid"]
    z = lambda a: np.where(fl, a, 0.0)
    u2 = F["ux"] * F["ux"] + F["uy"] * F["uy"]
    ke = 0.5 * F["rho"] * u2
    ens = 0.5 * F["vort"] * F["vort"]
    return dict(n_fluid=float(fl.sum()), sum_rho=total(z(F["rho"])), sum_ke=total(z(ke)), sum_diss=total(z(F["diss"])),
                sum_enstrophy=total(z(ens)), max_u2=float(z(u2).max()), max_gdot=float(z(F["gdot"]).max()),
                max_abs_div=float(z(np.abs(F["div"])).max()))


def expected(sim):
    """-> (fields, sums) for the handle's present state"""
    cfg = sim.config()
    w = sim.walls()
    F = fields(sim.f, sim.obst, sim.kinematics, w["Mgx"], w["Mby"], cfg.dx, cfg.c, cfg.phys.s8, cfg.phys.s9, cfg.nbgrains)
    return F, sums(F)


def mismatches(got, want, names=NAMES):
    """fields that are not array_equal (NaN never equals: a NaN anywhere is a finding)"""
    return [name for name in names if name in got and not np.array_equal(np.asarray(got[name]), want[name])]


def be_floats(a):
    return np.ascontiguousarray(a, dtype=np.float64).astype(np.float32).astype(">f4").tobytes()


def file_bytes(ux, uy, vort, gdot, diss):
    """flow%.6i.vtk as the header documents it, assembled here"""
    lx, ly = ux.shape
    pas = np.float32(1. / lx)
    out = b"# vtk DataFile Version 2.0\nWritten using VisIt writer\nBINARY\n"
    out += b"DATASET RECTILINEAR_GRID\nDIMENSIONS %d %d 1\n" % (lx, ly)
    out += b"X_COORDINATES %d float\n" % lx + (np.arange(lx, dtype=np.float32) * pas).astype(">f4").tobytes()
    out += b"Y_COORDINATES %d float\n" % ly + (np.arange(ly, dtype=np.float32) * pas).astype(">f4").tobytes()
    out += b"Z_COORDINATES 1 float\n" + struct.pack(">f", 0.0)
    out += b"CELL_DATA %d\nPOINT_DATA %d\n" % ((lx - 1) * (ly - 1), lx * ly)
    vec = np.zeros((ly, lx, 3))
    vec[:, :, 0] = ux.T
    vec[:, :, 1] = uy.T
    out += b"VECTORS fluid_velocity_lb float\n" + be_floats(vec)
    for name, p in (("vorticity", vort), ("shear_rate", gdot), ("dissipation", diss)):
        out += b"SCALARS %s float\nLOOKUP_TABLE default\n" % name.encode() + be_floats(p.T)
    return out


def data_line(t, s):
    return "%e" % t + "".join(" %e" % s[name] for name in SUMS) + "\n"
