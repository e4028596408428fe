#!/usr/bin/env python3
"""Generate tests/golden/densities_*.npz: what write_densities (lbmdem_write_densities, include/lbmdem_hip.h) must write,
from the UNMODIFIED reference.

The reference never calls write_densities (main.c:482-566) and its library does not export it, so the routine is restated
here over the reference's own f and obst: explicit loops over the directions i = 0..8 on float64 arrays, one rounding per
operation, in the reference's association; every value formatted with "%.4f" % float(v) -- like glibc's printf the correctly
rounded decimal of the exact binary value. Per case the golden holds the sha256 and the byte count of the two files, the byte
count of every file row of both sections, the text of file rows 0, 1, 2, ly / 2, ly - 1 of both sections and the text of
pressure_base. Data only is committed. Runs where the reference library can be built (pyoracle.Reference); one process per
case (the reference keeps its state in globals).

    python tests/golden/make_densities_golden.py
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

RHO_MOY = 1000.0                                # main.c:74
EX = (0, -1, -1, -1, 0, 1, 1, 1, 0)             # main.c:70
EY = (0, 1, 0, -1, -1, -1, 0, 1, 1)             # main.c:71
NFILE = 7                                       # the number in the two file names (any: it is not part of their text)


def cases():
    """name -> lattice, grains (mm) or sample, sub-steps (0: one obst_construction instead: a lattice at rest)"""
    import samples
    r, x, y = samples.row_packing(256, 200, 600, seed=77)    # L_b of make_links_golden.py: the G4 packing cropped
    keep = (x + r + 0.3 < 13.1) & (y + r + 0.3 < 9.6)
    return {
        "densities_La_37x50": dict(lx=37, ly=50, r_mm=np.array([0.62, 0.55, 0.70]), x_mm=np.array([0.35, 1.47, 2.60]),
                                   y_mm=np.array([1.30, 1.30, 4.75]), steps=0),
        "densities_Lc_64x61": dict(lx=64, ly=61, r_mm=np.array([0.80, 0.75, 0.85, 0.60]), x_mm=np.array([1.2, 3.2, 5.0, 1.5]),
                                   y_mm=np.array([1.2, 1.2, 1.2, 4.5]), steps=0),
        "densities_Lb_131x96": dict(lx=131, ly=96, r_mm=r[keep], x_mm=x[keep], y_mm=y[keep], steps=24),
        "densities_a08d83_98x119": dict(lx=98, ly=119, sample="a08d83.data", fluid_steps=24),
        "densities_a08d83_256x200": dict(lx=256, ly=200, sample="a08d83.data", fluid_steps=24),
    }


def sample_path(case, tmpdir):
    """the case's grains as a file in the reference's .data format"""
    if "sample" in case:
        return os.path.join(HERE, "ref_samples", case["sample"])
    import pyoracle as po
    p = os.path.join(tmpdir, "densities_case.data")
    po.write_sample(p, case["r_mm"], case["x_mm"], case["y_mm"], comment="#densities golden")
    return p


def grains_m(case):
    """(r, x1, x2) in metres, as the reference's reader parses them"""
    import pyoracle as po
    if "sample" in case:
        return po.read_sample(os.path.join(HERE, "ref_samples", case["sample"]))
    return tuple(np.asarray(case[k], float) * 1e-3 for k in ("r_mm", "x_mm", "y_mm"))


def substeps(case, npdem):
    return case["fluid_steps"] * npdem if "fluid_steps" in case else case["steps"]


def drive(sim, case, npdem, step="steps"):
    """the case's sequence on a pyoracle.Reference / Oracle (step = "renderScene": on a handle)"""
    n = substeps(case, npdem)
    if n:
        getattr(sim, step)(n)
    else:
        sim.obst_construction()


# ---- write_densities, restated -----------------------------------------------------------------------------------

def fields(f, obst):
    """main.c:524-528, 548-553 -> P, u_x, u_y as [lx][ly]; +0.0 where obst >= 0 (main.c:535, 559)"""
    P = np.zeros(obst.shape)
    ux = np.zeros(obst.shape)
    uy = np.zeros(obst.shape)
    with np.errstate(all="ignore"):
        for i in range(9):
            P = P + f[:, :, i]
        P = ((1. / 3.) * RHO_MOY) * (P - 1.)
        for i in range(9):
            ux = ux + f[:, :, i] * float(EX[i])
            uy = uy + f[:, :, i] * float(EY[i])
    fluid = obst < 0
    return np.where(fluid, P, 0.0), np.where(fluid, ux, 0.0), np.where(fluid, uy, 0.0)


def header(lx, ly, t=0.0):
    """main.c:498-520"""
    pas = 1. / lx
    xs = "".join("%e " % (float(np.float32(i)) * pas) for i in range(lx))
    ys = "".join("%e " % (float(np.float32(i)) * pas) for i in range(ly))
    return ("# vtk DataFile Version 2.0\nOutfile domain LB t: %e\nASCII\nDATASET RECTILINEAR_GRID\nDIMENSIONS %d %d 1\n"
            "X_COORDINATES %d float\n%s\nY_COORDINATES %d float\n%s\nZ_COORDINATES 1 float\n0\nPOINT_DATA %d\n"
            "SCALARS Pressure float 1\nLOOKUP_TABLE default\n" % (t, lx, ly, lx, xs, ly, ys, lx * ly))


VELOCITY_HEAD = "VECTORS VecVelocity float\n"


def rows(f, obst):
    """-> (pressure rows, velocity rows): per section the text of every file row (one y, all x), main.c:522-562"""
    P, ux, uy = fields(f, obst)
    prow = ["".join("%.4f\n" % float(v) for v in P[:, y]) for y in range(obst.shape[1])]
    vrow = ["".join("%.4f %.4f 0.\n" % (float(a), float(b)) for a, b in zip(ux[:, y], uy[:, y])) for y in range(obst.shape[1])]
    return prow, vrow


def pressure_base(f, obst):
    """main.c:531-538: "%le %le\\n" of x * pasxyz and P for row y == 2"""
    lx, ly = obst.shape
    if ly <= 2:
        return ""
    P = fields(f, obst)[0]
    pas = 1. / lx
    return "".join("%e %e\n" % (x * pas, float(P[x, 2])) for x in range(lx))


def files(f, obst, t=0.0):
    """-> the text of densities%.6i.vtk and of pressure_base%.6i.dat"""
    prow, vrow = rows(f, obst)
    return header(obst.shape[0], obst.shape[1], t) + "".join(prow) + VELOCITY_HEAD + "".join(vrow), pressure_base(f, obst)


def kept_rows(ly):
    return sorted({0, 1, 2, ly // 2, ly - 1})


def snapshot(f, obst):
    """what is committed"""
    prow, vrow = rows(f, obst)
    vtk, press = files(f, obst)
    res = dict(vtk_sha256=np.array(hashlib.sha256(vtk.encode()).hexdigest()), vtk_bytes=np.int64(len(vtk)),
               press_sha256=np.array(hashlib.sha256(press.encode()).hexdigest()), press_bytes=np.int64(len(press)),
               row_bytes=np.array([[len(s) for s in prow], [len(s) for s in vrow]], np.int64),
               press_text=np.frombuffer(press.encode(), np.uint8), solid_nodes=np.int64((obst >= 0).sum()),
               grain_nodes=np.int64((obst[1:-1, 1:-1] >= 0).sum()))
    for y in kept_rows(obst.shape[1]):
        res["p_row_%d" % y] = np.frombuffer(prow[y].encode(), np.uint8)
        res["v_row_%d" % y] = np.frombuffer(vrow[y].encode(), np.uint8)
    return res


def histogram(f, obst):
    """line length -> lines, per section"""
    prow, vrow = rows(f, obst)
    out = []
    for sec in (prow, vrow):
        h = {}
        for s in sec:
            for line in s.split("\n")[:-1]:
                h[len(line) + 1] = h.get(len(line) + 1, 0) + 1
        out.append(dict(sorted(h.items())))
    return out


def check_case(name, case, res):
    """what the case exists for, asserted on the golden"""
    assert res["grain_nodes"] > 0, (name, "no grain on the map")
    # (a lattice at rest prints 0.0000 and -0.0000: the sums of the equilibrium populations cancel to within an ulp)
    moving = any(bytes(res["v_row_%d" % y]).translate(None, b"-0. \n") for y in kept_rows(case["ly"]))
    assert moving == (substeps(case, 12) > 0), (name, "moving fluid", moving)
    assert res["row_bytes"].shape == (2, case["ly"]) and res["row_bytes"].sum() < res["vtk_bytes"]


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
        drive(R, case, R.scalars()["npDEM"])
        f, obst = R.get_f(), R.get_obst()
        res = snapshot(f, obst)
        hp, hv = histogram(f, obst)
        res["hist_pressure"] = np.array(sorted(hp.items()), np.int64).reshape(-1, 2)
        res["hist_velocity"] = np.array(sorted(hv.items()), np.int64).reshape(-1, 2)
        np.savez_compressed(sys.argv[3], **res)
        return
    for name, case in cases().items():
        res = generate(name)
        check_case(name, case, res)
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **res)
        print(name, "vtk bytes", int(res["vtk_bytes"]), "grain nodes", int(res["grain_nodes"]), "line lengths: pressure",
              dict(res["hist_pressure"].tolist()), "velocity", dict(res["hist_velocity"].tolist()), "file bytes",
              os.path.getsize(os.path.join(HERE, name + ".npz")))


if __name__ == "__main__":
    main()
