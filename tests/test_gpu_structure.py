"""GPU: the packing structure analysis (lbmdem_structure_compute and its readers, lbmdem_write_structure,
lbmdem_set_structure_output; include/lbmdem_hip.h) against the restatement over grain_table() (tests/structure_util.py): every
integer by array_equal, every double on the bits."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import contacts_util as cu
import packing_util as pu
import structure_util as su
from test_gpu_clusters import shape_packing, table_substep

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "2d-lbm-dem_amd", "host", "lbmdem")
REF_DIR = os.path.join(cu.HERE, "golden", "dem_G6_4000steps")
WHOLE = " needs the whole lattice and all grains on this handle (not a strip of a decomposition, no distributed grains)"
NO_COMPUTE = "%s: no lbmdem_structure_compute has been made for the grains where they are now"
COUNTS_ONLY = "%s: the last lbmdem_structure_compute had max_entries == 0: counts and histogram only"
READERS = ("lbmdem_download_structure_grains", "lbmdem_structure_grains_device", "lbmdem_download_structure_hist",
           "lbmdem_download_structure_neighbours")


def restatement_of(sim):
    t = sim.grain_table()
    return su.Restatement(t[:, 0], t[:, 1], t[:, 9])


def check(sim, A, rcut, nbins, shell):
    """one compute against the restatement A.at(...), every output -> the restatement"""
    R = A.at(rcut, nbins, shell)
    what = (sim.n, rcut, nbins, shell)
    counts = sim.structure(rcut, nbins, shell)
    assert counts == R["counts"], (what, counts, R["counts"])
    hist = sim.structure_hist()
    assert hist.dtype == np.int64 and np.array_equal(hist, R["hist"]), what
    off, nbr = sim.structure_neighbours()
    assert off.dtype == nbr.dtype == np.int32
    assert np.array_equal(off, R["offsets"]) and np.array_equal(nbr, R["nbr"]), what
    g = sim.structure_grains()
    for name in ("nb", "bonds"):
        assert np.array_equal(g[name], R["grains"][name]), (what, name)
    for name in ("c6", "s6", "c2", "s2"):
        assert su.same_bits(g[name], R["grains"][name]), (what, name, np.nonzero(g[name] != R["grains"][name])[0][:5])
    return R


def sweep(sim, A, big=True):
    """the four cutoffs, three bin counts and two shells of a scene"""
    n = sim.n
    D = 2.0 * float(A.r.mean())
    dmin = np.sqrt(A.d2[A.off_diagonal].min()) if n > 1 else D
    cuts = [0.5 * dmin, 1.1 * D, 3.3 * D] + ([1.0] if big else [])   # (a metre: larger than any box here)
    out = {}
    for rcut in cuts:
        for nbins in (1, 7, 4096):
            for shell in (1.0, 1.2):
                out[rcut, nbins, shell] = check(sim, A, rcut, nbins, shell)
    none, alle = out[cuts[0], 7, 1.2]["counts"], out[cuts[-1], 7, 1.2]["counts"]
    assert none["entries"] == 0 and none["lone_grains"] == n
    if big:
        assert alle["pairs"] == n * (n - 1) // 2
    return out


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 1025])
def test_shapes_against_the_restatement(pkg, n):
    lx, ly, r, x, y, k = shape_packing(n)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        table_substep(sim, k, 1)
        A = restatement_of(sim)
        out = sweep(sim, A, big=n <= 257)
        if n >= 63:
            mid = out[[c for c in out if c[1:] == (7, 1.2)][1][0], 7, 1.2]["counts"]
            assert mid["bonded_pairs"] >= 1 and mid["max_neighbours"] >= 2
        # the torch views are the downloads
        g = sim.structure_grains()
        tv = sim.structure_tensors()
        for name in su.STRUCTURE_DTYPE.names:
            assert tv[name].is_cuda and np.array_equal(tv[name].cpu().numpy().view(np.uint8), np.ascontiguousarray(g[name]).view(np.uint8))
        # any pointer may be NULL; sizing, and a buffer that is too small
        L = pkg.load_library()
        bonds = np.full(n, -1, np.int32)
        assert L.lbmdem_download_structure_grains(sim._h, None, bonds.ctypes.data_as(ctypes.c_void_p), None, None, None, None) == 0
        assert np.array_equal(bonds, g["bonds"])
        off, nbr = sim.structure_neighbours()
        cnt = ctypes.c_long(-1)
        assert L.lbmdem_download_structure_neighbours(sim._h, None, None, 0, ctypes.byref(cnt)) == 0 and cnt.value == len(nbr)
        if len(nbr) > 1:
            small = np.full(len(nbr) - 1, -7, np.int32)
            cnt.value = -1
            assert L.lbmdem_download_structure_neighbours(sim._h, None, small.ctypes.data_as(ctypes.c_void_p), len(small),
                                                          ctypes.byref(cnt)) == -1
            assert cnt.value == len(nbr) and (small == -7).all()
            assert "there are %d entries, the buffer holds %d" % (len(nbr), len(small)) in L.lbmdem_last_error().decode()


def test_shuffled_triangular_packing(pkg):
    """127 x 121 with the numbering shuffled: a grain's neighbours come out of the cells in any order but ascending"""
    r, x, y = pu.tri_packing_m(127, 121, 0.35, shuffle=True)
    with pkg.LbmDem(127, 121, r, x, y) as sim:
        table_substep(sim, None, 1)
        A = restatement_of(sim)
        out = sweep(sim, A)
        R = out[[c for c in out if c[1:] == (7, 1.2)][1][0], 7, 1.2]
        assert R["counts"]["six_bonds"] > sim.n // 3                 # the crystal
        psi6, _ = su.order_parameters(R["grains"])
        assert psi6 > 0.6


def ulp_placements(v):
    return [np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)]


@pytest.mark.parametrize("case", ["cutoff", "edge", "bond"])
def test_exact_thresholds_one_ulp_to_either_side(pkg, case):
    """two grains 2^-9 apart along x, radii 2^-10: d2 = 2^-18 is rc2 (rcut 2^-9), e2[2] (rcut 2^-8, four bins) and b*b (shell 1)"""
    x0, y0, rad = 2.0 ** -7, 2.0 ** -7, 2.0 ** -10
    rcut, nbins, shell = {"cutoff": (2.0 ** -9, 4, 1.2), "edge": (2.0 ** -8, 4, 1.2), "bond": (2.0 ** -8, 4, 1.0)}[case]
    outcome = {"cutoff": lambda R: R["counts"]["pairs"], "edge": lambda R: int(np.nonzero(R["hist"])[0][0]),
               "bond": lambda R: R["counts"]["bonded_pairs"]}[case]
    want = {"cutoff": [1, 1, 0], "edge": [1, 2, 2], "bond": [1, 1, 0]}[case]
    r = np.array([rad, rad])
    places = ulp_placements(x0 + 2.0 ** -9)
    # first the restatement alone: the three placements do not all come out the same, and the boundary is on the stated side
    for xb, w in zip(places, want):
        R = su.restate(np.array([x0, xb]), np.array([y0, y0]), r, rcut, nbins, shell)
        assert outcome(R) == w, (case, xb)
    assert su.restate(np.array([x0, places[1]]), np.array([y0, y0]), r, rcut, nbins, shell)["e2"][2 if case != "cutoff" else 4] == 2.0 ** -18
    assert len(set(want)) > 1
    with pkg.LbmDem(256, 200, r, [x0, places[1]], [y0, y0]) as sim:
        table_substep(sim, None, 1)
        for xb, w in zip(places, want):
            k = sim.kinematics
            k[:, 0], k[:, 1] = [x0, xb], [y0, y0]
            sim.kinematics = k
            A = restatement_of(sim)
            assert A.x[1] == xb and A.d2[0, 1] == (xb - x0) * (xb - x0)
            R = check(sim, A, rcut, nbins, shell)
            assert outcome(R) == w, (case, xb)


def test_special_centres(pkg):
    """coincident centres, a NaN and an infinite centre, and a grain far off the lattice, all in one scene"""
    lx, ly, r, x, y, k = shape_packing(65)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        table_substep(sim, k, 1)
        k = sim.kinematics
        k[10, 0:2] = k[3, 0:2]
        k[11, 0:2] = k[3, 0:2]
        k[5, 0] = np.nan
        k[7, 1] = np.inf
        k[8, 0] = -np.inf
        k[20, 0:2] = [1e3, -1e3]
        sim.kinematics = k
        A = restatement_of(sim)
        D = 2.0 * float(A.r.mean())
        for rcut in (1.1 * D, 3.3 * D, 1.0):
            for nbins in (7, 4096):
                R = check(sim, A, rcut, nbins, 1.2)
                c = R["counts"]
                assert c["coincident_pairs"] == 3 and c["nonfinite_grains"] == 3
                assert (R["grains"]["nb"][[5, 7, 8, 20]] == 0).all()
        assert c["pairs"] == 61 * 60 // 2


def test_four_hundred_grains_in_one_cell(pkg):
    """more candidates in a cell than one staging round holds"""
    lx, ly, r, x, y, k = shape_packing(400)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        table_substep(sim, k, 1)
        k = sim.kinematics
        gx, gy = np.meshgrid(np.arange(20), np.arange(20))
        p = np.random.default_rng(2).permutation(400)
        k[:, 0], k[:, 1] = 5e-3 + 1e-5 * gx.ravel()[p], 5e-3 + 1e-5 * gy.ravel()[p]
        sim.kinematics = k
        A = restatement_of(sim)
        R = check(sim, A, 2.5e-4, 7, 1.2)          # the whole blob is one cell, and not every pair is inside the cutoff
        assert 400 * 399 // 2 > R["counts"]["pairs"] > 400 * 300 // 2 and R["counts"]["max_neighbours"] == 399
        R = check(sim, A, 4e-5, 4096, 1.0)         # several cells with a few dozen each
        assert R["counts"]["bonded_pairs"] == R["counts"]["pairs"] > 400 * 10


def test_max_entries(pkg):
    lx, ly, r, x, y, k = shape_packing(65)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        table_substep(sim, k, 1)
        A = restatement_of(sim)
        rcut = 3.3 * 2.0 * float(A.r.mean())
        R = check(sim, A, rcut, 7, 1.2)
        need = R["counts"]["entries"]
        assert need > 10
        assert sim.structure(rcut, 7, 1.2, max_entries=need) == R["counts"]
        with pytest.raises(pkg.LbmDemError) as e:
            sim.structure(rcut, 7, 1.2, max_entries=need - 1)
        assert e.value.code == -1
        assert sim._L.lbmdem_last_error().decode() == ("lbmdem_structure_compute: the list has %d entries, max_entries is %d"
                                                       % (need, need - 1))
        for who, call in zip(READERS, (sim.structure_grains, sim.structure_tensors, sim.structure_hist, sim.structure_neighbours)):
            with pytest.raises(pkg.LbmDemError):
                call()
            assert sim._L.lbmdem_last_error().decode() == NO_COMPUTE % who     # a refused compute is none
        assert sim.structure(rcut, 7, 1.2, max_entries=0) == R["counts"]       # counts and histogram only
        assert np.array_equal(sim.structure_hist(), R["hist"])
        for who, call in ((READERS[0], sim.structure_grains), (READERS[1], sim.structure_tensors), (READERS[3], sim.structure_neighbours)):
            with pytest.raises(pkg.LbmDemError):
                call()
            assert sim._L.lbmdem_last_error().decode() == COUNTS_ONLY % who
        for bad in (-1, 2 ** 31):
            with pytest.raises(pkg.LbmDemError, match="max_entries must lie in 0 .. 2147483647"):
                sim.structure(rcut, 7, 1.2, max_entries=bad)
        for kw in (dict(rcut=0.0), dict(rcut=float("nan")), dict(rcut=float("inf")), dict(rcut=rcut, nbins=0),
                   dict(rcut=rcut, nbins=4097), dict(rcut=rcut, shell=0.99), dict(rcut=rcut, shell=float("inf"))):
            with pytest.raises(pkg.LbmDemError, match="rcut must be finite and > 0|nbins must lie in 1 .. 4096|shell must be finite and >= 1"):
                sim.structure(**kw)
        check(sim, A, rcut, 7, 1.2)


def test_readers_refuse_before_a_compute_and_after_a_move(pkg):
    lx, ly, r, x, y, k = shape_packing(65)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        calls = (sim.structure_grains, sim.structure_tensors, sim.structure_hist, sim.structure_neighbours)

        def refused():
            for who, call in zip(READERS, calls):
                with pytest.raises(pkg.LbmDemError) as e:
                    call()
                assert e.value.code == -1 and sim._L.lbmdem_last_error().decode() == NO_COMPUTE % who
        refused()                                   # after create
        table_substep(sim, k, 1)
        refused()
        rcut = 1.1 * 2.0 * float(np.mean(r))
        check(sim, restatement_of(sim), rcut, 7, 1.2)
        sim.dem_substep()
        refused()                                   # after a sub-step
        check(sim, restatement_of(sim), rcut, 7, 1.2)
        sim.renderScene(1)
        refused()                                   # after a coupled step
        sim.set_diagnostics(True)
        sim.dem_substep()
        check(sim, restatement_of(sim), rcut, 7, 1.2)
        sim.kinematics = sim.kinematics
        refused()                                   # after an upload of kinematics
        check(sim, restatement_of(sim), rcut, 7, 1.2)
        sim.structure_hist()                        # reading does not invalidate


def test_analysis_does_not_interfere(pkg, tmp_path):
    z = np.load(os.path.join(REF_DIR, "inputs_and_table.npz"))
    r, x, y = z["r_mm"] * 1e-3, z["x_mm"] * 1e-3, z["y_mm"] * 1e-3
    rcut = 3.3 * 2.0 * float(r.mean())
    with pkg.LbmDem(256, 200, r, x, y) as a, pkg.LbmDem(256, 200, r, x, y) as b:
        for piece in (1, 7, 3, 13):
            a.renderScene(piece); b.renderScene(piece)
            a.structure(rcut, 64, 1.2); a.structure_grains(); a.structure_neighbours(); a.structure(rcut / 3, 7, 1.0, max_entries=0)
            a.write_structure(str(tmp_path), piece, rcut, 16, 1.2)
        assert a.nbsteps == b.nbsteps == 24
        for what in ("f", "obst", "kinematics", "fhf"):
            assert np.array_equal(getattr(a, what), getattr(b, what)), what


@pytest.fixture(scope="module")
def g6_scene(pkg, tmp_path_factory):
    """the G6 golden through run_scene to step 4000, with the structure output on and without"""
    z = np.load(os.path.join(REF_DIR, "inputs_and_table.npz"))
    r, x, y = z["r_mm"] * 1e-3, z["x_mm"] * 1e-3, z["y_mm"] * 1e-3
    rcut, nbins, shell = 3.3 * 2.0 * float(r.mean()), 32, 1.2
    with_dir, without_dir = tmp_path_factory.mktemp("with"), tmp_path_factory.mktemp("without")
    with pkg.LbmDem(256, 200, r, x, y) as sim:
        sim.run_scene(4000, str(without_dir))
    with pkg.LbmDem(256, 200, r, x, y) as sim:
        sim.set_structure_output(True, rcut, nbins, shell)
        sim.run_scene(4000, str(with_dir))
        A = restatement_of(sim)
        R = check(sim, A, rcut, nbins, shell)
        got = dict(grains=sim.structure_grains(), hist=sim.structure_hist(), counts=sim.structure(rcut, nbins, shell),
                   t=sim.nbsteps * sim.config().dt, W=sim.config().Mdx - sim.config().Mgx, H=sim.config().Mhy - sim.config().Mby)
    return dict(z=z, rcut=rcut, nbins=nbins, shell=shell, with_dir=with_dir, without_dir=without_dir, R=R, got=got)


def test_g6_at_4000_through_run_scene(pkg, g6_scene, tmp_path):
    S = g6_scene
    new = ["structure000000.dat", "gr000000.dat", "structure.data"]
    others = sorted(os.listdir(S["without_dir"]))
    assert sorted(os.listdir(S["with_dir"])) == sorted(others + new) and "DEM000000.dat" in others
    for name in others:
        assert (S["with_dir"] / name).read_bytes() == (S["without_dir"] / name).read_bytes(), name
    got = S["got"]
    assert got["counts"] == S["R"]["counts"] and got["counts"]["pairs"] > 100
    pkg.write_structure_files(str(tmp_path), 0, got["grains"], S["rcut"], S["nbins"], S["shell"], got["hist"], got["counts"], got["t"],
                              got["W"], got["H"])
    for name in new:
        assert (S["with_dir"] / name).read_bytes() == (tmp_path / name).read_bytes(), name
    want = su.files_text(S["R"]["grains"], S["rcut"], S["nbins"], S["shell"], S["R"]["hist"], S["R"]["counts"], got["t"], got["W"], got["H"])
    assert (S["with_dir"] / "structure000000.dat").read_text() == want[0]
    assert (S["with_dir"] / "gr000000.dat").read_text() == want[1]
    assert (S["with_dir"] / "structure.data").read_text() == su.DATA_HEADER + want[2]


def test_host_driver_writes_the_structure_files(po, g6_scene, tmp_path):
    """`lbmdem <G6> --steps 4001 --structure RCUT --structure-bins N --structure-shell S` in a child process"""
    S, z = g6_scene, g6_scene["z"]
    sample = tmp_path / "packing.data"
    po.write_sample(str(sample), z["r_mm"], z["x_mm"], z["y_mm"])
    out = subprocess.run([EXE, str(sample), "--lx", "256", "--ly", "200", "--steps", "4001", "--structure", repr(S["rcut"]),
                          "--structure-bins", str(S["nbins"]), "--structure-shell", repr(S["shell"])], capture_output=True, text=True,
                         cwd=tmp_path, timeout=600)
    assert out.returncode == 0, out.stderr[-600:]
    for name in ("structure000000.dat", "gr000000.dat", "structure.data"):
        assert (tmp_path / name).read_bytes() == (S["with_dir"] / name).read_bytes(), name
    refused = subprocess.run([EXE, str(sample), "--structure", "2e-3", "--gpus", "2"], capture_output=True, text=True, cwd=tmp_path,
                             timeout=120)
    assert refused.returncode != 0 and "--structure is a single-GPU mode" in refused.stderr


def test_refusals(pkg):
    lx, ly, r, x, y, k = shape_packing(65)
    rcut = 2e-3
    if os.path.exists(pkg.SP_LIB_PATH):
        with pkg.LbmDem(lx, ly, r, x, y, precision="f32") as sp:
            for call in (lambda: sp.structure(rcut), sp.structure_grains, sp.structure_tensors, sp.structure_hist,
                         sp.structure_neighbours, lambda: sp.write_structure(".", 0, rcut), lambda: sp.set_structure_output(True, rcut)):
                with pytest.raises(pkg.LbmDemError) as e:
                    call()
                assert e.value.code == -1
                assert sp._L.lbmdem_last_error().decode() == ("the packing structure analysis is not available in the "
                                                              "single-precision build of the library")

    def text(sim, call):
        with pytest.raises(pkg.LbmDemError) as e:
            call()
        assert e.value.code == -1, e.value
        return sim._L.lbmdem_last_error().decode()
    with pkg.LbmDem(lx, ly, r, x, y, strip=(lx // 2, lx), halo=12) as strip:
        for who, call in (("lbmdem_structure_compute", lambda: strip.structure(rcut)),
                          ("lbmdem_download_structure_grains", strip.structure_grains),
                          ("lbmdem_download_structure_hist", strip.structure_hist),
                          ("lbmdem_download_structure_neighbours", strip.structure_neighbours),
                          ("lbmdem_structure_compute", lambda: strip.write_structure(".", 0, rcut)),
                          ("lbmdem_set_structure_output", lambda: strip.set_structure_output(True, rcut))):
            assert text(strip, call) == who + WHOLE
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        sim.set_structure_output(True, rcut)
        assert text(sim, sim.dist_enable) == ("the packing structure analysis is not available with distributed grains "
                                              "(lbmdem_set_structure_output(h, 0, 0., 0, 0.) first)")
        sim.set_structure_output(False)
        sim.dist_enable()
        for who, call in (("lbmdem_set_structure_output", lambda: sim.set_structure_output(True, rcut)),
                          ("lbmdem_structure_compute", lambda: sim.structure(rcut)),
                          ("lbmdem_structure_compute", lambda: sim.write_structure(".", 0, rcut))):
            assert text(sim, call) == who + WHOLE
