"""CPU: the two-dimensional packings of tests/packing_util.py.

1. The scenes the packed GPU tests (tests/test_gpu_packed.py) and the packed golden case run on are what they are for: most
   grains carry three or more touching partners, most contact normals are steep, the overlaps are a packing's, nothing lies
   outside the lattice. Conditions on the INPUTS, from numpy alone -- rows (samples.row_packing) fail the first two.
2. The in-repo oracle against the unmodified reference, live, on two such packings (the mechanism of
   tests/test_oracle_vs_reference.py: one spawned process per case, skipped where the reference cannot be built): "GPU equals
   oracle" on these scenes is then a chain that ends at the reference."""
import multiprocessing as mp

import numpy as np
import pytest

import contacts_util as cu
import packing_util as pu
import samples

# every lattice / mean radius / numbering the packed tests use (spread: pu.spread_of; noise 0.003 mm; default_rng(7))
SCENES = [(256, 200, 0.7), (127, 121, 0.5), (256, 200, 0.35), (98, 119, 0.6), (200, 150, 0.6), (203, 122, 0.5), (687, 122, 0.5)]


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("lx,ly,rmean", SCENES)
def test_scenes_are_many_contact_packings(lx, ly, rmean, shuffle):
    r, x, y = pu.tri_packing(lx, ly, rmean, shuffle=shuffle)
    c = pu.check_scene(lx, ly, r, x, y, (lx, ly, rmean))
    print(f"{lx} x {ly}, rmean {rmean}: {c}")
    assert c["grains"] >= 80 and c["touching_pairs"] > c["grains"]      # more contacts than grains: impossible in rows
    # the triangular lattice: nothing but the numbering depends on `shuffle`
    r0, x0, y0 = pu.tri_packing(lx, ly, rmean)
    o, o0 = np.lexsort((y, x)), np.lexsort((y0, x0))
    assert np.array_equal(r[o], r0[o0]) and np.array_equal(x[o], x0[o0]) and np.array_equal(y[o], y0[o0])
    assert shuffle == (not np.array_equal(x, x0))


def test_generator_lays_a_triangular_lattice():
    lx, ly, rmean = 256, 200, 0.7
    r, x, y = pu.tri_packing(lx, ly, rmean, spread=0.0, noise=0.0)
    assert len(r) == 280 and (r == rmean).all()
    rows = np.unique(np.round(y, 9))
    assert len(rows) == 16 and np.allclose(np.diff(rows), 2 * rmean * np.sqrt(3) / 2)
    first = [x[np.isclose(y, v)].min() for v in rows]
    assert np.allclose(first[0::2], 0.05 + rmean) and np.allclose(first[1::2], 0.05 + 2 * rmean)      # odd rows: half a pitch
    assert np.allclose(np.diff(np.sort(x[np.isclose(y, rows[0])])), 2 * rmean)
    assert x.min() - rmean >= 0.05 - 1e-12 and x.max() + rmean <= 0.1 * lx - 0.05 + 1e-12
    assert y.min() - rmean >= 0.05 - 1e-12 and y.max() + rmean <= 0.1 * ly - 0.05 + 1e-12
    # the draws: radii within the spread, the jitter small, n_max keeps the first grains
    r, x2, y2 = pu.tri_packing(lx, ly, rmean)
    assert np.abs(r - rmean).max() <= 0.01 and 0 < np.abs(x2 - x).max() < 0.02 and 0 < np.abs(y2 - y).max() < 0.02
    assert np.allclose(pu.tri_packing(lx, ly, rmean, n_max=100, spread=0.0, noise=0.0)[1], x[:100])
    # every third grain of the bottom row 2 um into the floor
    rp, xp, yp = pu.tri_packing(lx, ly, rmean, floor_push=True)
    pushed = np.nonzero(yp != y2)[0]
    assert np.array_equal(pushed, np.arange(0, 18, 3)) and np.array_equal(yp[pushed], rp[pushed] - 0.002)
    pu.check_scene(lx, ly, rp, xp, yp, "floor push")


def test_rows_are_not_such_a_scene():
    """what the new inputs add: in samples.row_packing no grain has a third touching partner and no normal is steep"""
    r, x, y = samples.row_packing(1024, 640, 2500, seed=5)
    c = pu.census(1024, 640, r, x, y)
    assert c["frac_3_partners"] == 0.0 and c["frac_steep"] == 0.0 and c["touching_pairs"] < c["grains"], c
    with pytest.raises(AssertionError):
        pu.check_scene(1024, 640, r, x, y)


def test_reduced_discs_meet_many_partners():
    """tests/test_gpu_packed.py's map test: at reductionR 1.08 at least 30 % of the grains have three or more partners whose
    reduced disc meets theirs (rows: two at the most)"""
    r, x, y = pu.tri_packing(200, 150, 0.6)
    assert (pu.reduced_disc_partners(r, x, y, 1.08) >= 3).mean() >= 0.30
    rr, xr, yr = samples.row_packing(200, 150, 60, seed=8)
    assert pu.reduced_disc_partners(rr, xr, yr, 1.08).max() <= 2


def contact_counts(po, lx, ly, r, x1, x2, k, nbsteps):
    """the counters of the contact export for a table sub-step from k, from the restatement and the oracle's pair list alone"""
    ora = po.Oracle(lx, ly, r, x1, x2)
    ora.set_kinematics(k)
    ora.verlet_rebuild()
    s = ora.scalars()
    P = cu.params(s["dt"], s["dt2"], s["Mgx"], s["Mdx"], s["Mby"], s["Mhy"])
    wf = cu.wallflags_of_lists(len(r), ora.verlet()[3])
    return cu.restate(k, r, ora.pairs(), wf, P, nbsteps % cu.PHYSICS["stepFilm"] == 0)[1]


@pytest.mark.parametrize("nbsteps", [0, 1])
def test_contact_scene_has_the_counts_the_gpu_test_asks_for(po, nbsteps):
    """the kicks of test_gpu_packed's contact export case give more contacts than grains, clamped and force-free contacts
    and wall contacts by the restatement alone (nbsteps 0: the film law)"""
    lx, ly, r, x1, x2, k = pu.contact_scene()
    counts = contact_counts(po, lx, ly, r, x1, x2, k, nbsteps)
    print(nbsteps, counts)
    assert counts["touching_pairs"] >= len(r) and counts["coulomb_clamped"] > 0 and counts["fn_zero"] > 0, counts
    assert counts["wall_contacts"] >= 6


def _worker(lx, ly, path, nsteps, q):
    import pyoracle as po
    try:
        R = po.Reference(lx, ly, path)
        O = po.Oracle.from_file(path, lx, ly)
        k = pu.agitation(R.n)
        k[:, 0:2] = R.get_grains()[:, 0:2]
        R.set_kinematics(k); O.set_kinematics(k)
        bad = []
        if R.scalars() != O.scalars(): bad.append("scalars")
        if not np.array_equal(R.rlb(), O.rlb()): bad.append("rLB")
        if not np.array_equal(R.get_obst(), O.get_obst()): bad.append("init_obst")
        for chunk in (1, nsteps - 1):
            R.steps(chunk); O.steps(chunk)
            for key in ("f", "obst", "act", "delta", "fhf"):
                if not np.array_equal(getattr(R, "get_" + key)(), getattr(O, "get_" + key)()): bad.append(key)
            gr, go = R.get_grains(), O.get_grains()
            bad += [n for n, c in po.COL.items() if not np.array_equal(gr[:, c], go[:, c], equal_nan=True)]
            rv, ov = R.verlet(), O.verlet()
            npairs = int(rv[0].max())
            if not (np.array_equal(rv[0], ov[0]) and np.array_equal(rv[1][:npairs], ov[1][:npairs])
                    and np.array_equal(rv[2], ov[2]) and all(np.array_equal(a, b) for a, b in zip(rv[3], ov[3]))):
                bad.append("verlet")
            if R.total_density() != O.total_density(): bad.append("total_density")
        moved = float(np.abs(go[:, 0:2] - k[:, 0:2]).max())
        q.put((bad, O.act_anomalies(), npairs, moved))
    except Exception as e:  # pragma: no cover
        q.put(([repr(e)], -1, -1, 0.0))


@pytest.mark.parametrize("lx,ly,rmean,shuffle", [(127, 121, 0.5, False), (98, 119, 0.6, True)])
def test_oracle_bit_equal_to_reference_on_a_packing(po, tmp_path, lx, ly, rmean, shuffle):
    """every field tests/test_oracle_vs_reference.py compares, after 1 and after 131 sub-steps (the list is rebuilt behind
    sub-step 100), from agitated grains: sums over three and more partners, steep normals, any numbering"""
    if po.build_ref(lx, ly) is None:
        pytest.skip("reference sources not present (GPU box): the oracle is pinned by tests/golden there")
    r, x, y = pu.tri_packing(lx, ly, rmean, shuffle=shuffle)
    pu.check_scene(lx, ly, r, x, y, (lx, ly))
    path = str(tmp_path / "packing.data")
    po.write_sample(path, r, x, y, comment="#triangular packing")
    nsteps = 131
    q = mp.get_context("spawn").Queue()
    p = mp.get_context("spawn").Process(target=_worker, args=(lx, ly, path, nsteps, q))
    p.start()
    bad, anomalies, npairs, moved = q.get(timeout=600)
    p.join()
    assert bad == [], f"fields differing from the reference: {bad}"
    assert anomalies == 0 and npairs > 2 * len(r), (anomalies, npairs)
    assert moved > 1e-6, moved      # the grains did move (more than a micron): the contacts of the later sub-steps are not the first ones
