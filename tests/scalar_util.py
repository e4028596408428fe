"""The passive scalar (include/lbmdem_hip.h: lbmdem_scalar_set, lbmdem_scalar_step, lbmdem_scalar_sums, lbmdem_write_scalar_files)
restated in numpy, bit for bit: elementwise float64 operations are IEEE operations, one rounding each, so an expression written
with the header's association IS the header's value. The velocity planes are those of the flow fields (flow_util.fields over the
handle's downloads: f, obst, kinematics, walls(), config()); the scalar's own state is scalar_state()."""
import numpy as np

import flow_util as fu

W = (1. / 3, 1. / 6, 1. / 6, 1. / 6, 1. / 6)
E = ((0, 0), (-1, 0), (0, -1), (1, 0), (0, 1))   # q = 0, 2, 4, 6, 8 of the fluid's set
OPP = (0, 3, 4, 1, 2)
SUMS = ("n_fluid", "sum_C", "sum_C2", "min_C", "max_C")
DATA_HEADER = "# step n_fluid sum_C sum_C2 min_C max_C\n"


def diffusivity(tau_s):
    return (tau_s - 0.5) / 3.


def conc(g):
    """C = (((g0 + g1) + g2) + g3) + g4"""
    return g[..., 0] + g[..., 1] + g[..., 2] + g[..., 3] + g[..., 4]


def at(a, dx, dy, fill):
    """b[x][y] = a[x + dx][y + dy], `fill` where that lies outside the lattice"""
    lx, ly = a.shape
    b = np.full_like(a, fill)
    xs, xd = (slice(max(dx, 0), lx + min(dx, 0)), slice(max(-dx, 0), lx + min(-dx, 0)))
    ys, yd = (slice(max(dy, 0), ly + min(dy, 0)), slice(max(-dy, 0), ly + min(-dy, 0)))
    b[xd, yd] = a[xs, ys]
    return b


def initial(C, obst):
    """lbmdem_scalar_set -> (g, was)"""
    fluid = obst == -1
    g = np.zeros(C.shape + (5,))
    for k in range(5):
        g[..., k] = np.where(fluid, W[k] * C, 0.0)
    return g, fluid


def refill(g, was, obst):
    """stage 1 -> (g with the uncovered nodes filled, the number of eligible neighbours of every uncovered node, -1 elsewhere)"""
    fluid = obst == -1
    elig = fluid & was
    stored = conc(g)
    S = np.zeros(obst.shape)
    cnt = np.zeros(obst.shape, np.int64)
    with np.errstate(all="ignore"):
        for k in range(1, 5):
            e = at(elig, E[k][0], E[k][1], False)
            S = S + np.where(e, at(stored, E[k][0], E[k][1], 0.0), 0.0)   # (S is never -0.0: adding +0.0 is skipping)
            cnt += e
        Cf = np.where(cnt > 0, S / np.maximum(cnt, 1), 0.0)
    need = fluid & ~was
    out = g.copy()
    for k in range(5):
        out[..., k] = np.where(need, W[k] * Cf, g[..., k])
    return out, np.where(need, cnt, -1)


def step(g, was, obst, ux, uy, omega):
    """one step -> (g, was)"""
    fluid = obst == -1
    g1, _ = refill(g, was, obst)
    with np.errstate(all="ignore"):
        C = conc(g1)
        a0 = W[0] * C
        a = W[1] * C
        s = (None, -ux, -uy, ux, uy)
        eq = [a0] + [a * (1. + 3. * s[k]) for k in range(1, 5)]
        gs = [g1[..., k] - omega * (g1[..., k] - eq[k]) for k in range(5)]
    out = np.zeros_like(g)
    for k in range(5):
        ex, ey = E[k]
        src_fluid = at(fluid, -ex, -ey, False)
        pulled = np.where(src_fluid, at(gs[k], -ex, -ey, 0.0), gs[OPP[k]])
        out[..., k] = np.where(fluid, pulled, 0.0)
    return out, fluid.copy()


def planes(sim):
    """-> (ux, uy) of the flow-fields block for the handle's present state"""
    cfg = sim.config()
    w = sim.walls()
    F = fu.fields(sim.f, sim.obst, sim.kinematics, w["Mgx"], w["Mby"], cfg.dx, cfg.c, cfg.phys.s8, cfg.phys.s9, cfg.nbgrains)
    return F["ux"], F["uy"]


def expected_step(sim, omega, uv=None):
    """the handle's present scalar stepped once in its present state -> (g, was, C)"""
    ux, uy = uv if uv is not None else planes(sim)
    g, was = sim.scalar_state()
    g2, was2 = step(g, was, sim.obst, ux, uy, omega)
    return g2, was2, conc(g2)


def sums(g, was):
    """lbmdem_scalar_sums -> dict of SUMS"""
    C = conc(g)
    n = int(was.sum())
    with np.errstate(all="ignore"):
        sq = C * C
    lo = float(C[was].min()) if n else 0.0
    hi = float(C[was].max()) if n else 0.0
    return dict(n_fluid=float(n), sum_C=fu.total(np.where(was, C, 0.0)), sum_C2=fu.total(np.where(was, sq, 0.0)), min_C=lo, max_C=hi)


def data_line(step_count, s):
    return "%e" % float(step_count) + "".join(" %e" % s[name] for name in SUMS) + "\n"


def file_bytes(C):
    """scalar%.6i.vtk as the header documents it, assembled here"""
    lx, ly = C.shape
    pas = float(np.float32(1. / lx))
    out = b"# vtk DataFile Version 2.0\nlbmdem passive scalar\nBINARY\nDATASET STRUCTURED_POINTS\n"
    out += b"DIMENSIONS %d %d 1\nORIGIN 0 0 0\nSPACING %s %s 1\n" % (lx, ly, b"%.9g" % pas, b"%.9g" % pas)
    out += b"POINT_DATA %d\nSCALARS concentration float\nLOOKUP_TABLE default\n" % (lx * ly)
    with np.errstate(over="ignore"):
        out += np.ascontiguousarray(C.T, dtype=np.float64).astype(np.float32).astype(">f4").tobytes()
    return out
