#!/usr/bin/env python3
"""Generate tests/golden/probes_*.npz: what the probe recorder (lbmdem_probe_*, include/lbmdem_hip.h) must record, from
the UNMODIFIED reference.

The reference's diagnostic routines (write_densities main.c:522-541, velocity_profile main.c:1647-1676, pressures
main.c:1681-1694, xgrainmax / height of write_DEM main.c:400-405) are never called and not exported by the reference
library, so their formulas are restated here over the reference's own f, obst and grain table: explicit loops over the
directions i = 0..8 on float64 arrays, one rounding per operation, in the reference's association. Data only is
committed. Runs where the reference library can be built (pyoracle.Reference); one process per case (the reference keeps
its state in globals).

    python tests/golden/make_probe_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

RHO_MOY = 1000.0                                # main.c:74
EY = (0, 1, 0, -1, -1, -1, 0, 1, 1)             # main.c:71
FIELDS = ("step", "time", "velocity_y", "velocity_row", "point_pressure", "xgrainmax", "height")


def cases():
    """name -> lattice, sample, fluid steps, the pressure rows recorded (one run of the reference serves them all; a
    handle records one), the nodes of `pressures`. Row 2 is the reference's own; row 12 goes through the bottom grains of
    the G4 packing, row 14 through those of a08d83."""
    import samples
    r, x, y = samples.row_packing(256, 200, 600, seed=77)    # G4's packing (tests/golden/make_golden.py)
    pts = ((1, 1), (40, 2), (128, 100), (200, 150), (254, 198), (0, 50), (31, 12), (100, 30))
    return {
        "probes_G4_256x200": dict(lx=256, ly=200, r_mm=r, x_mm=x, y_mm=y, fluid_steps=30, pressure_rows=(2, 12), points=pts),
        "probes_a08d83_256x200": dict(lx=256, ly=200, sample="a08d83.data", fluid_steps=24, pressure_rows=(2, 14), points=pts),
    }


def sample_path(case, tmpdir):
    """the case's grains as a file in the reference's .data format"""
    if "sample" in case:
        return os.path.join(HERE, "ref_samples", case["sample"])
    import pyoracle as po
    p = os.path.join(tmpdir, "probe_case.data")
    po.write_sample(p, case["r_mm"], case["x_mm"], case["y_mm"], comment="#probe golden")
    return p


def grains_m(case):
    """(r, x1, x2) in metres, as the reference's reader parses them"""
    import pyoracle as po
    if "sample" in case:
        return po.read_sample(os.path.join(HERE, "ref_samples", case["sample"]))
    return tuple(np.asarray(case[k], float) * 1e-3 for k in ("r_mm", "x_mm", "y_mm"))


# ---- the five formulas, restated --------------------------------------------------------------------------------

def pressure_row(f, obst, y):
    """main.c:524-539 for one y: P = 0.; P += f[x][y][i]; P = (1. / 3.) * rho_moy * (P - 1.) where obst < 0, else 0.0"""
    P = np.zeros(f.shape[0])
    for i in range(9):
        P = P + f[:, y, i]
    P = ((1. / 3.) * RHO_MOY) * (P - 1.)
    return np.where(obst[:, y] < 0, P, 0.0)


def velocity_row(f, obst, grains, sc, nbgrains):
    """main.c:1658-1672 -> (y, u_y1[lx], nodes that took the grain branch)"""
    y = int((grains[0, 1] - sc["Mby"]) / sc["dx"])
    d_loc = np.zeros(f.shape[0])
    u_y = np.zeros(f.shape[0])
    for i in range(9):
        d_loc = d_loc + f[:, y, i]
    for i in range(9):
        u_y = u_y + f[:, y, i] * float(EY[i])
    o = obst[:, y]
    on_grain = (o != -1) & (o != nbgrains)
    with np.errstate(divide="ignore", invalid="ignore"):
        fluid = u_y / d_loc
    grain = grains[np.where(on_grain, o, 0), 4] / sc["c"]
    return y, np.where(on_grain, grain, fluid), int(on_grain.sum())


def point_pressure(f, obst, points):
    """main.c:1685-1691 at the given nodes"""
    c_squ = 1. / 3.
    out = np.zeros(len(points))
    for k, (x, y) in enumerate(points):
        if obst[x, y] == -1:
            s = f[x, y, 0]
            for i in range(1, 9):
                s = s + f[x, y, i]
            out[k] = (s - RHO_MOY) * c_squ
    return out


def extent(grains, rcol):
    """main.c:400-405"""
    return float(np.max(grains[:, 0] + grains[:, rcol])), float(np.max(grains[:, 1] + grains[:, rcol]))


def sample_now(sim, case):
    """The record of the fluid step the backend is about to make (its counter is a multiple of npDEM): the grain table
    first -- the fluid step sees the grains as the sub-step before left them --, then one renderScene, whose DEM sub-step
    touches neither f nor obst. `sim`: pyoracle.Reference or anything with its method names."""
    import pyoracle as po
    sc = sim.scalars()
    s = sim.nbsteps
    grains = sim.get_grains()
    sim.steps(1)
    f, obst = sim.get_f(), sim.get_obst()
    y, vrow, on_grain = velocity_row(f, obst, grains, sc, len(grains))
    xg, hg = extent(grains, po.COL["r"])
    rec = dict(step=s, time=s * sc["dt"], velocity_y=y, velocity_row=vrow, point_pressure=point_pressure(f, obst, case["points"]),
               xgrainmax=xg, height=hg, velocity_on_grain=on_grain)
    for row in case["pressure_rows"]:
        rec[f"pressure_row_{row}"] = pressure_row(f, obst, row)
        rec[f"pressure_solid_{row}"] = int((obst[1:-1, row] >= 0).sum())   # interior nodes of the row that took the 0.0 branch
    return rec


def run_case(sim, case):
    """-> dict of arrays, one row per fluid step"""
    npdem = sim.scalars()["npDEM"]
    recs = []
    for _ in range(case["fluid_steps"]):
        recs.append(sample_now(sim, case))
        sim.steps(npdem - 1)
    return {k: np.array([r[k] for r in recs]) for k in recs[0]}


def generate(name):
    """the case on the reference, in a process of its own -> dict of arrays"""
    import subprocess
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "case.npz")
        subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, out], check=True, stdout=subprocess.DEVNULL)
        return dict(np.load(out))


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--case":   # (the child process of generate)
        import tempfile
        import pyoracle as po
        case = cases()[sys.argv[2]]
        with tempfile.TemporaryDirectory() as tmp:
            R = po.Reference(case["lx"], case["ly"], sample_path(case, tmp))
        np.savez_compressed(sys.argv[3], **run_case(R, case))
        return
    for name in cases():
        res = generate(name)
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **res)
        print(name, {k: v.shape for k, v in res.items()}, "velocity nodes on grains:", int(res["velocity_on_grain"].sum()),
              {k: int(v.sum()) for k, v in res.items() if k.startswith("pressure_solid")})


if __name__ == "__main__":
    main()
