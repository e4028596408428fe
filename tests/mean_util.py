"""The time-averaged flow statistics (include/lbmdem_hip.h: lbmdem_mean_sample, lbmdem_mean_fields, lbmdem_mean_profile,
lbmdem_write_mean_files) restated in numpy, bit for bit: elementwise float64 operations are IEEE operations, one rounding each, so
an expression written with the header's association IS the header's value. A sample's addends are the planes of the flow fields
(flow_util.fields over the handle's downloads: f, obst, kinematics, walls(), config()) plus the map's classes; np.where picks, per
node, the sum with the addend or the sum as it was -- the header's "left untouched"."""
import struct

import numpy as np

import flow_util as fu

U, UU, RHO, DISS, GRAIN = 1, 2, 4, 8, 16
ALL = 31
PLANES = (("Sux", "Suy"), ("Sxx", "Sxy", "Syy"), ("Srho", "Srho2"), ("Sdiss", "Sgdot"), ("Sgux", "Sguy"))   # per bit of the mask
FIELDS = ("phi", "solid", "mux", "muy", "rxx", "rxy", "ryy", "mrho", "vrho", "mdiss", "mgdot", "gux", "guy")
FALL = 8191
NEEDS = dict(phi=0, solid=0, mux=U, muy=U, rxx=U | UU, rxy=U | UU, ryy=U | UU, mrho=RHO, vrho=RHO, mdiss=DISS, mgdot=DISS,
             gux=GRAIN, guy=GRAIN)
PROFILE_ROWS = FIELDS + ("nf",)
PROFILE_HEADER = "# y samples phi solid mux muy rxx rxy ryy mrho vrho mdiss mgdot gux guy\n"


def plane_names(mask):
    return [name for k, group in enumerate(PLANES) if mask >> k & 1 for name in group]


def fmask_of(names):
    return sum(1 << FIELDS.index(n) for n in names)


def window(shape, mask=ALL):
    """an open window: the selected planes +0.0, the counts 0"""
    acc = {name: np.zeros(shape) for name in plane_names(mask)}
    acc["n_fluid"] = np.zeros(shape, np.uint32)
    acc["n_grain"] = np.zeros(shape, np.uint32)
    return acc


def state(sim):
    """-> the planes of the flow-fields block for the handle's present state, with the grains' nodes"""
    cfg = sim.config()
    w = sim.walls()
    obst = sim.obst
    F = fu.fields(sim.f, obst, sim.kinematics, w["Mgx"], w["Mby"], cfg.dx, cfg.c, cfg.phys.s8, cfg.phys.s9, cfg.nbgrains)
    F["grain"] = (obst >= 0) & (obst < cfg.nbgrains)
    return F


def sample(acc, F):
    """one sample of the planes F (ux, uy, rho, diss, gdot, fluid, grain) into the window `acc`, in place"""
    fl, gr = F["fluid"], F["grain"]
    assert not (fl & gr).any()
    ux, uy, rho = F["ux"], F["uy"], F["rho"]
    with np.errstate(all="ignore"):
        fluid_addends = dict(Sux=ux, Suy=uy, Sxx=ux * ux, Sxy=ux * uy, Syy=uy * uy, Srho=rho, Srho2=rho * rho, Sdiss=F["diss"],
                             Sgdot=F["gdot"])
        for name, v in fluid_addends.items():
            if name in acc:
                acc[name] = np.where(fl, acc[name] + v, acc[name])
        for name, v in dict(Sgux=ux, Sguy=uy).items():
            if name in acc:
                acc[name] = np.where(gr, acc[name] + v, acc[name])
    acc["n_fluid"] = acc["n_fluid"] + fl.astype(np.uint32)
    acc["n_grain"] = acc["n_grain"] + gr.astype(np.uint32)
    return acc


def available(acc):
    """the derived fields the window's planes give"""
    have = sum(1 << k for k, group in enumerate(PLANES) if group[0] in acc)
    return [name for name in FIELDS if not NEEDS[name] & ~have]


def derived(acc, samples):
    """-> {name: plane} of all thirteen derived fields; +0.0 where the divisor count is 0 and for a field the window cannot give"""
    N = float(samples)
    nf, ng = acc["n_fluid"].astype(np.float64), acc["n_grain"].astype(np.float64)
    zero = np.zeros(nf.shape)

    def over(name, n):
        with np.errstate(all="ignore"):
            return np.where(n > 0, acc[name] / np.where(n > 0, n, 1.0), 0.0)

    have = available(acc)
    D = {name: zero.copy() for name in FIELDS}
    D["phi"], D["solid"] = nf / N, ng / N
    with np.errstate(all="ignore"):
        if "mux" in have:
            D["mux"], D["muy"] = over("Sux", nf), over("Suy", nf)
        if "rxx" in have:
            D["rxx"] = np.where(nf > 0, over("Sxx", nf) - D["mux"] * D["mux"], 0.0)
            D["rxy"] = np.where(nf > 0, over("Sxy", nf) - D["mux"] * D["muy"], 0.0)
            D["ryy"] = np.where(nf > 0, over("Syy", nf) - D["muy"] * D["muy"], 0.0)
        if "mrho" in have:
            D["mrho"] = over("Srho", nf)
            D["vrho"] = np.where(nf > 0, over("Srho2", nf) - D["mrho"] * D["mrho"], 0.0)
        if "mdiss" in have:
            D["mdiss"], D["mgdot"] = over("Sdiss", nf), over("Sgdot", nf)
        if "gux" in have:
            D["gux"], D["guy"] = over("Sgux", ng), over("Sguy", ng)
    return D


def profile(D, n_fluid):
    """-> (14, ly): per y the chain from +0.0 over x ascending of each derived plane, then of nf"""
    with np.errstate(all="ignore"):
        rows = [fu.chain(D[name], 0) for name in FIELDS] + [fu.chain(n_fluid.astype(np.float64), 0)]
    return np.stack(rows)


def file_bytes(phi, mux, muy, rxx, rxy, ryy, mrho):
    """mean%.6i.vtk as the header documents it, assembled here"""
    lx, ly = phi.shape
    pas = np.float32(1. / lx)
    out = b"# vtk DataFile Version 2.0\nWritten using VisIt writer\nBINARY\n"
    out += b"DATASET RECTILINEAR_GRID\nDIMENSIONS %d %d 1\n" % (lx, ly)
    out += b"X_COORDINATES %d float\n" % lx + (np.arange(lx, dtype=np.float32) * pas).astype(">f4").tobytes()
    out += b"Y_COORDINATES %d float\n" % ly + (np.arange(ly, dtype=np.float32) * pas).astype(">f4").tobytes()
    out += b"Z_COORDINATES 1 float\n" + struct.pack(">f", 0.0)
    out += b"CELL_DATA %d\nPOINT_DATA %d\n" % ((lx - 1) * (ly - 1), lx * ly)
    vec = np.zeros((ly, lx, 3))
    vec[:, :, 0] = mux.T
    vec[:, :, 1] = muy.T
    with np.errstate(all="ignore"):
        out += b"VECTORS mean_fluid_velocity_lb float\n" + fu.be_floats(vec)
        for name, p in (("fluid_fraction", phi), ("fluctuation_energy", 0.5 * (rxx + ryy)), ("reynolds_xy", rxy), ("mean_density", mrho)):
            out += b"SCALARS %s float\nLOOKUP_TABLE default\n" % name.encode() + fu.be_floats(p.T)
    return out


def profile_text(prof, samples, lx):
    """mean_profile%.6i.dat as the header documents it"""
    lines = [PROFILE_HEADER]
    for y in range(prof.shape[1]):
        lines.append("%d %d" % (y, samples) + "".join(" %e" % (float(prof[k, y]) / float(lx)) for k in range(len(FIELDS))) + "\n")
    return "".join(lines).encode()
