"""The fluid tracers (include/lbmdem_hip.h: lbmdem_tracer_advance, lbmdem_tracer_sample, lbmdem_write_tracers_files) restated in
numpy, bit for bit: elementwise float64 operations are IEEE operations, one rounding each, so an expression written one operation
per line with the header's association IS the header's value. The velocity planes are those of the flow fields (flow_util.fields
over the handle's downloads: f, obst, kinematics, walls(), config())."""
import numpy as np

import flow_util as fu


def planes(sim):
    """-> (ux, uy), the composite velocity of the handle's present state, [lx][ly] each"""
    cfg = sim.config()
    w = sim.walls()
    F = fu.fields(sim.f, sim.obst, sim.kinematics, w["Mgx"], w["Mby"], cfg.dx, cfg.c, cfg.phys.s8, cfg.phys.s9, cfg.nbgrains)
    return F["ux"], F["uy"]


def clamp(v, last):
    """!(v >= 0.) ? 0. : (v > (double)last ? (double)last : v): a NaN goes to 0"""
    with np.errstate(invalid="ignore"):
        return np.where(~(v >= 0.), 0., np.where(v > float(last), float(last), v))


def cells(px, py, lx, ly):
    """-> (i, j): (int)px lowered to lx - 2, (int)py lowered to ly - 2"""
    return np.minimum(px.astype(np.int64), lx - 2), np.minimum(py.astype(np.int64), ly - 2)


def velocity(ux, uy, px, py):
    """-> (U, V) at the points (px, py) of the domain"""
    lx, ly = ux.shape
    i, j = cells(px, py, lx, ly)
    a = px - i
    b = py - j
    with np.errstate(all="ignore"):
        ma = 1. - a
        mb = 1. - b
        w00 = ma * mb
        w10 = a * mb
        w01 = ma * b
        w11 = a * b
        out = []
        for u in (ux, uy):
            t00 = w00 * u[i, j]
            t10 = w10 * u[i + 1, j]
            t01 = w01 * u[i, j + 1]
            t11 = w11 * u[i + 1, j + 1]
            s = t00 + t10
            s = s + t01
            s = s + t11
            out.append(s)
    return out[0], out[1]


def advance(ux, uy, xy):
    """one advance of the positions xy, (n, 2) -> the new positions"""
    lx, ly = ux.shape
    px = clamp(xy[:, 0], lx - 1)   # (the identity on what set_tracers accepts and an advance leaves)
    py = clamp(xy[:, 1], ly - 1)
    U0, V0 = velocity(ux, uy, px, py)
    with np.errstate(all="ignore"):
        hx = 0.5 * U0
        hy = 0.5 * V0
        qx = clamp(px + hx, lx - 1)
        qy = clamp(py + hy, ly - 1)
        U1, V1 = velocity(ux, uy, qx, qy)
        nx = clamp(px + U1, lx - 1)
        ny = clamp(py + V1, ly - 1)
    return np.stack([nx, ny], axis=1)


def sample(ux, uy, obst, xy):
    """-> (n, 3): U, V at the positions and the nearest node's owner as a double"""
    U, V = velocity(ux, uy, xy[:, 0], xy[:, 1])
    o = obst[(xy[:, 0] + 0.5).astype(np.int64), (xy[:, 1] + 0.5).astype(np.int64)].astype(np.float64)
    return np.stack([U, V, o], axis=1)


def expected_advance(sim, uv=None):
    """the handle's present positions advanced once in its present state (uv: planes(sim) made earlier for the same state)"""
    ux, uy = uv if uv is not None else planes(sim)
    return advance(ux, uy, sim.tracers)


def same(a, b):
    """the same doubles (positions are never NaN: the clamp sends a NaN to 0)"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and not np.isnan(a).any() and np.array_equal(a, b)


def grid_seeds(lx, ly, nx, ny):
    """the host driver's --tracers NXxNY: px = (i + 0.5) * (lx - 1) / NX, py likewise, x-major"""
    px = (np.arange(nx) + 0.5) * (lx - 1) / nx
    py = (np.arange(ny) + 0.5) * (ly - 1) / ny
    return np.stack([np.repeat(px, ny), np.tile(py, nx)], axis=1)


def be_floats(a):
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(a, dtype=np.float64).astype(np.float32).astype(">f4").tobytes()


def file_bytes(lx, xy, uvo):
    """tracers%.6i.vtk as the header documents it, assembled here"""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    uvo = np.asarray(uvo, np.float64).reshape(-1, 3)
    n = len(xy)
    pas = np.float32(1. / lx)
    pts = np.zeros((n, 3), np.float32)
    pts[:, 0] = xy[:, 0].astype(np.float32) * pas
    pts[:, 1] = xy[:, 1].astype(np.float32) * pas
    verts = np.stack([np.ones(n, np.int64), np.arange(n)], axis=1).astype(">i4")
    vec = np.zeros((n, 3))
    vec[:, :2] = uvo[:, :2]
    out = b"# vtk DataFile Version 2.0\nlbmdem fluid tracers\nBINARY\nDATASET POLYDATA\n"
    out += b"POINTS %d float\n" % n + pts.astype(">f4").tobytes()
    out += b"VERTICES %d %d\n" % (n, 2 * n) + verts.tobytes()
    out += b"POINT_DATA %d\nVECTORS tracer_velocity_lb float\n" % n + be_floats(vec)
    out += b"SCALARS tracer_owner float\nLOOKUP_TABLE default\n" + be_floats(uvo[:, 2])
    return out
