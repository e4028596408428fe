#!/usr/bin/env python3
"""Generate tests/golden/links_*.npz: what the boundary-link export (lbmdem_download_act, lbmdem_download_links,
lbmdem_geometry_stats; include/lbmdem_hip.h) must give, from the UNMODIFIED reference.

Per case the reference library of the case's lattice size is initialised with the case's grains, advanced by `steps`
renderScene calls, given the case's kinematics (if any) and asked for one more obst_construction (main.c:991-1065); its
obst, act, every non-zero delta entry (x, y, q, value) in the order of obst_writing's links.dat (main.c:1631-1639), the
grain table and the inputs are stored. Data only is committed. One process per case (the reference keeps its state in
globals).

An EFFECTIVE link is an entry the reference's bounce-back loop (main.c:1154-1222) interpolates: an interior node of a grain
with act == 1 whose neighbour in direction q is fluid. The other non-zero delta entries are STALE (left by a lower-index disc
where a higher-index disc painted later; never read). The generator asserts the number of stale entries per case: none in
the clean cases, some in the overlap case -- and the situations each case exists for.

    python tests/golden/make_links_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

EX = (0, -1, -1, -1, 0, 1, 1, 1, 0)    # main.c:70
EY = (0, 1, 0, -1, -1, -1, 0, 1, 1)    # main.c:71
LINK_DTYPE = np.dtype([("x", np.int32), ("y", np.int32), ("q", np.int32), ("grain", np.int32), ("delta", np.float64)])


def cases():
    """name -> lattice, grains (mm), renderScene calls, kinematics override (positions in mm; None: none), and what the
    generator asserts about the stale entries."""
    import samples
    # L_b: the G4 packing (tests/golden/make_golden.py) cropped to the lattice: 5 rows of 8 to 9 grains
    r, x, y = samples.row_packing(256, 200, 600, seed=77)
    keep = (x + r + 0.3 < 13.1) & (y + r + 0.3 < 9.6)
    return {
        # 37 x 50 (lx % 8 = 5; ly no multiple of 16 or 60): grain 0 clipped by the left wall, grain 2 by the top wall,
        # grains 0 and 1 exactly one fluid node apart on the row through their centres
        "links_La_37x50": dict(lx=37, ly=50, r_mm=np.array([0.62, 0.55, 0.70]), x_mm=np.array([0.35, 1.47, 2.60]),
                               y_mm=np.array([1.30, 1.30, 4.75]), steps=0, move_mm=None, clean=True),
        "links_Lb_131x96": dict(lx=131, ly=96, r_mm=r[keep], x_mm=x[keep], y_mm=y[keep], steps=24, move_mm=None, clean=True),
        # 64 x 61: created apart, then moved: reduced discs 0 and 1 overlap, 2 overlaps both (the three-disc `act` case),
        # 3 is free
        "links_Lc_64x61": dict(lx=64, ly=61, r_mm=np.array([0.80, 0.75, 0.85, 0.60]), x_mm=np.array([1.2, 3.2, 5.0, 1.5]),
                               y_mm=np.array([1.2, 1.2, 1.2, 4.5]), steps=0,
                               move_mm=(np.array([2.30, 3.10, 2.75, 4.90]), np.array([2.40, 2.40, 3.15, 4.60])), clean=False),
    }


def grains_m(case):
    return tuple(np.asarray(case[k], float) * 1e-3 for k in ("r_mm", "x_mm", "y_mm"))


def moved_kinematics(sim, case):
    """the case's kinematics: the sim's own with the positions replaced"""
    k = sim.get_grains()[:, :9].copy()
    k[:, 0] = case["move_mm"][0] * 1e-3
    k[:, 1] = case["move_mm"][1] * 1e-3
    return k


def drive(sim, case):
    """the case's sequence on a pyoracle.Reference, or anything with its method names"""
    if case["steps"]:
        sim.steps(case["steps"])
    if case["move_mm"] is not None:
        sim.set_kinematics(moved_kinematics(sim, case))
    sim.obst_construction()


def delta_entries(delta):
    """the non-zero entries of delta[lx][ly][9] in the order of links.dat (y outer, x inner, q = 1..8) -> x, y, q, value"""
    d = np.transpose(delta, (1, 0, 2))           # [y][x][q]
    yy, xx, qq = np.nonzero(d[:, :, 1:] != 0)    # (row-major: y, then x, then q)
    return xx.astype(np.int32), yy.astype(np.int32), (qq + 1).astype(np.int32), d[yy, xx, qq + 1]


def effective_links(obst, act, delta, n):
    """the effective links of a geometry in the order of links.dat, as LINK_DTYPE (a delta of exactly zero: q negated).
    `delta`: [lx][ly][9]."""
    lx, ly = obst.shape
    out = []
    interior = np.zeros((lx, ly), bool)
    interior[1:-1, 1:-1] = True
    solid = interior & (obst != -1) & (obst != n) & (act == 1)
    for q in range(1, 9):
        nb = np.full((lx, ly), n, obst.dtype)    # obst[x + ex][y + ey] (only asked at interior nodes)
        xs = slice(max(0, -EX[q]), lx - max(0, EX[q])); xd = slice(max(0, EX[q]), lx - max(0, -EX[q]))
        ys = slice(max(0, -EY[q]), ly - max(0, EY[q])); yd = slice(max(0, EY[q]), ly - max(0, -EY[q]))
        nb[xs, ys] = obst[xd, yd]
        xx, yy = np.nonzero(solid & (nb == -1))
        rec = np.zeros(len(xx), LINK_DTYPE)
        rec["x"], rec["y"], rec["grain"], rec["delta"] = xx, yy, obst[xx, yy], delta[xx, yy, q]
        rec["q"] = np.where(rec["delta"] != 0, q, -q)
        out.append(rec)
    out = np.concatenate(out)
    return out[np.lexsort((np.abs(out["q"]), out["x"], out["y"]))]


def census(obst, act, links, n):
    """the six counters of lbmdem_geometry_stats from a geometry and its effective links"""
    lx, ly = obst.shape
    interior = np.zeros((lx, ly), bool)
    interior[1:-1, 1:-1] = True
    solid = interior & (obst != -1) & (obst != n)
    active = solid & (act == 1)
    d = links["delta"]
    return [int(solid.sum()), int(active.sum()), len(links), int(((d > 0) & (d < 0.5)).sum()), int((d >= 0.5).sum()),
            8 * int(active.sum()) - len(links)]


def stale_count(res):
    """non-zero reference delta entries that are no effective links"""
    n = len(res["r_mm"])
    delta = np.zeros(res["obst"].shape + (9,))
    delta[res["delta_x"], res["delta_y"], res["delta_q"]] = res["delta_v"]
    eff = effective_links(res["obst"], res["act"].astype(np.int32), delta, n)
    eff = eff[eff["q"] > 0]
    have = set(zip(res["delta_x"].tolist(), res["delta_y"].tolist(), res["delta_q"].tolist()))
    assert all(k in have for k in zip(eff["x"].tolist(), eff["y"].tolist(), eff["q"].tolist()))
    return len(have) - len(eff)


def snapshot(sim, case):
    obst, act, delta = sim.get_obst(), sim.get_act(), sim.get_delta()
    dx_, dy_, dq_, dv_ = delta_entries(delta)
    return dict(obst=obst.astype(np.int32), act=act.astype(np.int8), delta_x=dx_, delta_y=dy_, delta_q=dq_, delta_v=dv_,
                grains=sim.get_grains(), r_mm=np.asarray(case["r_mm"], float), x_mm=np.asarray(case["x_mm"], float),
                y_mm=np.asarray(case["y_mm"], float), steps=np.int64(case["steps"]),
                move_mm=np.zeros((2, 0)) if case["move_mm"] is None else np.asarray(case["move_mm"], float))


def check_case(name, case, res):
    """what the case exists for, asserted on the reference's own arrays"""
    n, obst, act = len(case["r_mm"]), res["obst"], res["act"]
    stale = stale_count(res)
    assert (stale == 0) if case["clean"] else (stale > 0), (name, "stale delta entries", stale)
    assert sorted(set(obst[1:-1, 1:-1].ravel().tolist()) - {-1}) == list(range(n)), (name, "every grain is on the map")
    if name.startswith("links_La"):
        assert (obst[1, 1:-1] == 0).any() and (obst[1:-1, -2] == 2).any(), "clipped by the left and by the top wall"
        assert ((obst[:-2] == 0) & (obst[1:-1] == -1) & (obst[2:] == 1)).any(), "grains 0 and 1 one fluid node apart"
    if name.startswith("links_Lb"):
        assert len(res["delta_v"]) > 3000 and n >= 35
    if name.startswith("links_Lc"):
        inside = act[1:-1, 1:-1][(obst[1:-1, 1:-1] != -1)]
        assert (inside == 0).any() and (inside == 1).any()
        import pyoracle as po   # (the three-disc situation: the two-disc rule alone would get some node wrong)
        r, x1, x2 = grains_m(case)
        ora = po.Oracle(case["lx"], case["ly"], r, x1, x2)
        drive(ora, case)
        assert ora.act_anomalies() > 0, "no node needs the lowest-cover record"
    return stale


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
            p = os.path.join(tmp, "links_case.data")
            po.write_sample(p, case["r_mm"], case["x_mm"], case["y_mm"], comment="#links golden")
            R = po.Reference(case["lx"], case["ly"], p)
        drive(R, case)
        np.savez_compressed(sys.argv[3], **snapshot(R, case))
        return
    for name, case in cases().items():
        res = generate(name)
        stale = check_case(name, case, res)
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **res)
        print(name, "grains", len(case["r_mm"]), "non-zero delta entries", len(res["delta_v"]), "stale", stale,
              "bytes", os.path.getsize(os.path.join(HERE, name + ".npz")))


if __name__ == "__main__":
    main()
