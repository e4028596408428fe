#!/usr/bin/env python3
"""Generate tests/golden/contacts_*.npz: what the contact network export (lbmdem_download_contacts, lbmdem_contact_stats;
include/lbmdem_hip.h) must add up to, from the UNMODIFIED reference.

The reference declares `struct contact` (main.c:167-174) and never fills it, and its harness has no per-contact accessor: the
golden pins the contacts through the per-grain sums the reference accumulates from them in every sub-step -- p, s, f1, f2, ifm,
M11..M22, z, zz (main.c:1733-1745, 776-799, 830-838, 875-882, 907-915, 938-949, 1397-1416). Per case the reference library of
the case's lattice size is initialised with the case's grains, advanced by `steps` renderScene calls, given the case's
kinematics and step counter (if any) and a Verlet rebuild; the state at that moment (9 kinematic columns, step counter,
scalars, pair list, wall lists) is the PRE-STATE. One more renderScene call, and the 30-column grain table is stored with it.
Data only is committed. One process per case (the reference keeps its state in globals).

What each case exists for is asserted here, on the table where the table shows it and otherwise with the tests' numpy
restatement of the laws (tests/contacts_util.py) applied to the pre-state.

    python tests/golden/make_contacts_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def cases():
    """name -> lattice, grains (mm), initial velocities (make_golden's generator for the case, or none), renderScene calls, and
    what happens to the state before the pre-state is taken"""
    import golden_util as gu
    g5, g6 = gu.ALL_CASES["G5_dem_64x48"], gu.ALL_CASES["G6_output_256x200"]
    return {
        # the G5 packing with its random initial velocities after 120 calls. (The reference's own table shows one touching pair
        # and no grain on a wall at that moment -- the four wall grains have bounced off by call 60 --, so the walls are left to
        # the two cases below.)
        "contacts_Ca_64x48": dict(lx=64, ly=48, r_mm=g5["r_mm"], x_mm=g5["x_mm"], y_mm=g5["y_mm"], kin0=g5, steps=120,
                                  engineer=False, nbsteps=None),
        # the G6 packing after 240 calls; then the grains are put back where they were created (moving as they move by then),
        # one touching pair is pulled apart fast enough for fn to clamp to 0, another is sheared fast enough for the Coulomb clamp, and grain 0 is put into the bottom left corner with grain 1 leaning on it
        "contacts_Cb_256x200": dict(lx=256, ly=200, r_mm=g6["r_mm"], x_mm=g6["x_mm"], y_mm=g6["y_mm"], kin0=None, steps=240,
                                    engineer=True, nbsteps=None),
        # the same pre-state on a film step (main.c:1342): the inline law, which leaves f1, f2, ifm, zz alone
        "contacts_Cfilm_256x200": dict(lx=256, ly=200, r_mm=g6["r_mm"], x_mm=g6["x_mm"], y_mm=g6["y_mm"], kin0=None, steps=240,
                                       engineer=True, nbsteps=8000),
    }


def engineered(k, case, sim):
    """Cb's kinematics override, from the reference's own state after `steps` calls. Deterministic: the first touching pair of
    the list is pulled apart, the first touching pair that shares no grain with it is sheared."""
    import contacts_util as cu
    k = k.copy()
    n = len(k)
    r = np.asarray(case["r_mm"], float) * 1e-3
    # After 240 calls nothing touches any more: the packing's initial overlaps (a few micrometres) have pushed the grains apart.
    # The override therefore puts every grain back where it was created -- overlaps, the four grains pressed into the walls --
    # and keeps the velocities and accelerations the 240 calls have given it.
    k[:, 0], k[:, 1] = np.asarray(case["x_mm"], float) * 1e-3, np.asarray(case["y_mm"], float) * 1e-3
    s = sim.scalars()
    P = cu.params(s["dt"], s["dt2"], s["Mgx"], s["Mdx"], s["Mby"], s["Mhy"])
    # a grain with three contacts (a row packing has at most one per lower grain): grain 0, the first of the bottom row, at
    # rest in the corner, 2 um into the left and into the bottom wall, and grain 1 leaning on it 2 um deep, 10 um above the floor
    k[0, 0], k[0, 1] = P["Mgx"] + r[0] - 2e-6, P["Mby"] + r[0] - 2e-6
    d = r[0] + r[1] - 2e-6
    k[1, 1] = P["Mby"] + r[1] + 1e-5
    k[1, 0] = k[0, 0] + np.sqrt(d * d - (k[1, 1] - k[0, 1]) ** 2)
    k[:2, 2:] = 0.
    cumul, neigh, _, _ = sim.verlet()
    rec, _ = cu.pair_records(cu.advance(k, P), r, cu.pairs_of_list(cumul, neigh), P, False)
    rec = rec[(rec["i"] >= 2) & (rec["j"] < n - 4)]
    a = rec[0]
    b = rec[(rec["i"] != a["i"]) & (rec["i"] != a["j"]) & (rec["j"] != a["i"]) & (rec["j"] != a["j"])][0]
    for g in (a["i"], a["j"], b["i"], b["j"]):
        k[g, 3:] = 0.
    # fn = -kg dn - nug vn < 0 <=> vn > kg |dn| / nug: twice that, along the normal (it points from j to i)
    vn = 2. * P["kg"] * abs(a["dn"]) / P["nug"]
    k[a["i"], 3], k[a["i"], 4] = vn * a["nx"], vn * a["ny"]
    # |kt vt dt| > mu fn <=> |vt| > mu fn / (kt dt): four times that, along the tangent (-ny, nx)
    vt = 4. * P["mu"] * b["fn"] / (P["kt"] * P["dt"])
    k[b["i"], 3], k[b["i"], 4] = -vt * b["ny"], vt * b["nx"]
    return k, (int(a["i"]), int(a["j"])), (int(b["i"]), int(b["j"]))


def check_case(name, case, res):
    """what the case exists for, asserted on what is stored"""
    import contacts_util as cu
    n = len(case["r_mm"])
    P, film = cu.case_params(res), cu.case_film(res)
    assert film == (case["nbsteps"] == 8000)
    pairs = cu.pairs_of_list(res["cumul"], res["neigh"])
    rec, counts = cu.restate(res["pre"], res["r"], pairs, res["wallflags"], P, film)
    table = res["table"]
    # the restatement and the reference agree on this case (the tests ask the same of the device's records)
    bad = cu.table_mismatches(cu.replay(rec, table[:, 0], table[:, 1], n, film, P["dt"], P["mu"]), table)
    assert not bad, (name, "the restatement's records do not add up to the reference's table", bad)
    z = table[:, cu.TABLE_COLS["z"]]
    walls = set(rec["j"][rec["j"] < 0].tolist())
    assert counts["touching_pairs"] > 0, (name, counts)
    if case["engineer"]:
        assert walls == {cu.WALL_B, cu.WALL_T, cu.WALL_L, cu.WALL_R}, (name, walls)
        assert (table[n - 4:, cu.TABLE_COLS["p"]] != 0).all(), (name, "the four wall grains carry a normal force")
        assert (z == 0).any() and (z == 1).any() and (z >= 3).any(), (name, np.bincount(z.astype(int)))
        pr = rec[rec["j"] >= 0]
        pulled, sheared = tuple(res["pulled"]), tuple(res["sheared"])
        a = pr[(pr["i"] == pulled[0]) & (pr["j"] == pulled[1])]
        assert len(a) == 1 and a["fn"][0] == 0 and a["dn"][0] < 0, (name, "the pulled pair touches with fn clamped to 0", a)
        if not film:
            _, clamp = cu.pair_records(cu.advance(res["pre"], P), res["r"], pairs, P, film)
            b = (pr["i"] == sheared[0]) & (pr["j"] == sheared[1])
            assert b.sum() == 1 and clamp[b][0] and pr["fn"][b][0] > 0, (name, "the sheared pair takes the Coulomb clamp")
        assert counts["fn_zero"] >= 1 and counts["coulomb_clamped"] >= 1, (name, counts)
    if film:
        for c in ("f2", "ifm", "zz"):   # (f1 still takes the walls' share, main.c:832, 914, 939)
            assert not table[:, cu.TABLE_COLS[c]].any(), (name, c, "is left alone by the film law")
    return counts


def generate(name):
    """the case on the reference, in a process of its own -> dict of arrays"""
    import subprocess
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "case.npz")
        subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, out], check=True, stdout=subprocess.DEVNULL)
        return dict(np.load(out))


def run_case(case):
    import tempfile
    import contacts_util as cu
    import golden_util as gu
    import pyoracle as po
    with tempfile.TemporaryDirectory() as tmp:
        p = os.path.join(tmp, "contacts_case.data")
        po.write_sample(p, case["r_mm"], case["x_mm"], case["y_mm"], comment="#contacts golden")
        R = po.Reference(case["lx"], case["ly"], p)
    if case["kin0"] is not None:
        R.set_kinematics(gu.mg.dem_initial_kinematics(case["kin0"]))
    R.steps(case["steps"])
    pulled = sheared = (-1, -1)
    if case["engineer"]:
        R.verlet_rebuild()   # (the list the override picks its pairs from)
        k, pulled, sheared = engineered(R.get_grains()[:, :9], case, R)
        R.set_kinematics(k)
    if case["nbsteps"] is not None:
        R.set_nbsteps(case["nbsteps"])
    R.verlet_rebuild()
    g = R.get_grains()
    s = R.scalars()
    cumul, neigh, _, wl = R.verlet()
    res = dict(pre=g[:, :9].copy(), r=g[:, 9].copy(), nbsteps=np.int64(R.nbsteps),
               scalars=np.array([s[k] for k in po.SCALARS], float), cumul=cumul.astype(np.int32),
               neigh=neigh[:int(cumul[-2])].astype(np.int32), wallflags=cu.wallflags_of_lists(R.n, wl).astype(np.int8),
               pulled=np.array(pulled, np.int32), sheared=np.array(sheared, np.int32),
               r_mm=np.asarray(case["r_mm"], float), x_mm=np.asarray(case["x_mm"], float), y_mm=np.asarray(case["y_mm"], float))
    R.steps(1)
    res["table"] = R.get_grains()
    return res


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--case":   # (the child process of generate)
        np.savez_compressed(sys.argv[3], **run_case(cases()[sys.argv[2]]))
        return
    for name, case in cases().items():
        res = generate(name)
        counts = check_case(name, case, res)
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **res)
        print(name, "grains", len(case["r_mm"]), counts, "bytes", os.path.getsize(os.path.join(HERE, name + ".npz")))


if __name__ == "__main__":
    main()
