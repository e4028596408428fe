"""GPU: the Voronoi analysis (lbmdem_voronoi_compute and its readers, lbmdem_write_voronoi, lbmdem_set_voronoi_output;
include/lbmdem_hip.h) against the restatement over grain_table() and the walls of config() (tests/voronoi_util.py): every integer by
array_equal, every double on the bits."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import contacts_util as cu
import packing_util as pu
import voronoi_util as vu
from test_gpu_clusters import shape_packing, table_substep

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "2d-lbm-dem_amd", "host", "lbmdem")
REF_DIR = os.path.join(cu.HERE, "golden", "dem_G6_4000steps")
WHOLE = " needs the whole lattice and all grains on this handle (not a strip of a decomposition, no distributed grains)"
NO_COMPUTE = "%s: no lbmdem_voronoi_compute has been made for the grains where they are now"
NO_LIST = "lbmdem_voronoi_compute: no lbmdem_structure_compute has been made for the grains where they are now"
COUNTS_ONLY = ("lbmdem_voronoi_compute: the last lbmdem_structure_compute had max_entries == 0: counts and histogram only, and the "
               "cells need its neighbour list")
READERS = ("lbmdem_download_voronoi_grains", "lbmdem_voronoi_grains_device", "lbmdem_download_voronoi_faces")
INTS, DOUBLES = ("faces", "walls", "nverts", "flags"), ("area", "perimeter", "phi", "R2")


def box_of(sim):
    c = sim.config()
    return c.Mgx, c.Mdx, c.Mby, c.Mhy


def restatement_of(sim):
    t = sim.grain_table()
    return vu.Restatement(t[:, 0], t[:, 1], t[:, 9], box_of(sim))


def check(sim, A, rcut):
    """one compute against the restatement A.at(rcut), every output -> the restatement"""
    R = A.at(rcut)
    what = (sim.n, rcut)
    counts = sim.voronoi(rcut)
    assert counts == R["counts"], (what, counts, R["counts"])
    g = sim.voronoi_grains()
    for name in INTS:
        assert g[name].dtype == np.int32 and np.array_equal(g[name], R["grains"][name]), (what, name,
                                                                                          np.nonzero(g[name] != R["grains"][name])[0][:5])
    for name in DOUBLES:
        assert vu.same_bits(g[name], R["grains"][name]), (what, name, np.nonzero(g[name] != R["grains"][name])[0][:5])
    off, src, length = sim.voronoi_faces()
    assert off.dtype == src.dtype == np.int32 and length.dtype == np.float64
    assert np.array_equal(off, R["foff"]) and np.array_equal(src, R["fsrc"]) and vu.same_bits(length, R["flen"]), what
    return R


def hugging_lattice(pkg, lx, ly, r, x, y):
    """the smallest lattice (64 nodes at least) whose box still holds the packing: no cell then reaches far beyond the grains"""
    dx = pkg.derive(lx, ly, r, 1.0).dx
    return max(64, int(math.ceil((x + r).max() / dx)) + 2), max(64, int(math.ceil((y + r).max() / dx)) + 2)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 1025])
def test_shapes_against_the_restatement(pkg, n):
    lx, ly, r, x, y, k = shape_packing(n)
    lx, ly = hugging_lattice(pkg, lx, ly, r, x, y)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        # a new handle: the walls are the lattice's, the centres the ones it was made with (the grain table comes with the first
        # table sub-step). The restatement first: incomplete cells at the smallest cutoff, none at the largest
        k0 = sim.kinematics
        assert vu.same_bits(k0[:, 0], x) and vu.same_bits(k0[:, 1], y)
        A = vu.Restatement(x, y, r, box_of(sim))
        D = 2.0 * float(A.r.mean())
        cuts = [1.1 * D, 3.3 * D, 10.0 * D]
        assert A.at(cuts[0])["counts"]["complete"] < n
        assert A.at(cuts[2])["counts"]["complete"] == n == A.at(cuts[2])["counts"]["cells"]
        for rcut in cuts:
            check(sim, A, rcut)
        # the first Verlet rebuild puts the right and the top wall at ten times the lattice (the reference's VerletWall): the cells
        # of the free surface reach far, and stay incomplete at every cutoff
        table_substep(sim, k, 1)
        A = restatement_of(sim)
        assert A.box[1] > 5 * lx * 1e-4 and A.at(cuts[2])["counts"]["complete"] < n
        for rcut in (cuts if n <= 257 else cuts[1:2]):
            R = check(sim, A, rcut)
        if n == 1:
            g = R["grains"][0]
            W, H = box_of(sim)[1] - box_of(sim)[0], box_of(sim)[3] - box_of(sim)[2]
            assert g["nverts"] == 4 and g["faces"] == 0 and g["walls"] == 15 and g["area"] == pytest.approx(W * H, rel=1e-14)
        else:
            assert R["counts"]["grain_faces"] >= 2 and R["counts"]["wall_faces"] >= 4
        # the torch views are the downloads
        g = sim.voronoi_grains()
        tv = sim.voronoi_tensors()
        for name in vu.VORONOI_DTYPE.names:
            assert tv[name].is_cuda and np.array_equal(tv[name].cpu().numpy().view(np.uint8), np.ascontiguousarray(g[name]).view(np.uint8))
        # any pointer may be NULL; sizing, and buffers that are one entry short
        L = pkg.load_library()
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        flags, phi = np.full(n, -1, np.int32), np.full(n, -1.0)
        assert L.lbmdem_download_voronoi_grains(sim._h, None, None, vp(phi), None, None, None, None, vp(flags)) == 0
        assert np.array_equal(flags, g["flags"]) and vu.same_bits(phi, g["phi"])
        assert L.lbmdem_download_voronoi_grains(sim._h, *([None] * 8)) == 0
        assert L.lbmdem_voronoi_grains_device(sim._h, *([None] * 8)) == 0
        off, src, length = sim.voronoi_faces()
        cnt = ctypes.c_long(-1)
        assert L.lbmdem_download_voronoi_faces(sim._h, None, None, None, 0, ctypes.byref(cnt)) == 0 and cnt.value == len(src) >= 4
        only = np.full(len(src), -9, np.int32)
        assert L.lbmdem_download_voronoi_faces(sim._h, None, vp(only), None, len(only), ctypes.byref(cnt)) == 0
        assert np.array_equal(only, src)
        small, cnt.value = np.full(len(src) - 1, -7, np.int32), -1
        assert L.lbmdem_download_voronoi_faces(sim._h, None, vp(small), None, len(small), ctypes.byref(cnt)) == -1
        assert cnt.value == len(src) and (small == -7).all()
        assert "there are %d faces, the buffers hold %d" % (len(src), len(small)) in L.lbmdem_last_error().decode()


def test_shuffled_triangular_packing(pkg):
    """127 x 121 with the numbering shuffled: a crystal, most cells hexagons"""
    r, x, y = pu.tri_packing_m(127, 121, 0.35, shuffle=True)
    with pkg.LbmDem(127, 121, r, x, y) as sim:
        table_substep(sim, None, 1)
        A = restatement_of(sim)
        D = 2.0 * float(A.r.mean())
        for rcut in (1.1 * D, 3.3 * D, 10.0 * D):
            R = check(sim, A, rcut)
        assert (R["grains"]["faces"] == 6).sum() > 0.7 * sim.n and R["counts"]["complete"] > 0.5 * sim.n


def upload(sim, x, y):
    k = sim.kinematics
    k[:, :] = 0.0
    k[:, 0], k[:, 1] = x, y
    sim.kinematics = k
    A = restatement_of(sim)
    assert vu.same_bits(A.x, x) and vu.same_bits(A.y, y)
    return A


def test_square_lattice_of_equal_discs(pkg):
    """8 x 7 equal discs at spacing 2^-9: every inner vertex is shared by four cells, the clipping leaves edges of no length there
    (in some cells; which, the order of the neighbours decides), and they are no faces"""
    a = 2.0 ** -9
    gx, gy = np.meshgrid(np.arange(1, 9) * a, np.arange(1, 8) * a)
    p = np.random.default_rng(3).permutation(gx.size)
    x, y = gx.ravel()[p], gy.ravel()[p]
    r = np.full(len(x), 2.0 ** -11)
    with pkg.LbmDem(256, 200, r, x, y) as sim:
        table_substep(sim, None, 1)
        A = upload(sim, x, y)
        inner = (x > 1.5 * a) & (x < 7.5 * a) & (y > 1.5 * a) & (y < 6.5 * a)
        for rcut in (1.5 * a, 4 * a):
            g = A.at(rcut)["grains"]
            assert (g["faces"][inner] == 4).all() and (g["walls"][inner] == 0).all()
            assert (np.abs(g["area"][inner] - a * a) <= 4 * np.finfo(float).eps * a * a).all()   # (at most eight terms of 2^-19)
            assert (g["nverts"][inner] > 4).any()            # edges of no length are there, and are not counted
            check(sim, A, rcut)


def test_lattice_vertex_one_ulp_to_either_side(pkg):
    """nine grains of radius 2^-11, the centre at (2^-6, 2^-6), spacing 2^-9; the diagonal neighbour (+, +) one ulp below, at, and
    above its place: the centre's cell has 5, 4, 4 faces and the area 2^-18 in all three"""
    a, c = 2.0 ** -9, 2.0 ** -6
    places = (np.nextafter(c + a, -np.inf), c + a, np.nextafter(c + a, np.inf))

    def nine(dd):
        return (np.array([c, c + a, c - a, c, c, dd, c - a, c + a, c - a]), np.array([c, c, c, c + a, c - a, dd, c + a, c - a, c - a]))
    r = np.full(9, 2.0 ** -11)
    with pkg.LbmDem(256, 200, r, *nine(c + a)) as sim:
        table_substep(sim, None, 1)
        for dd, faces in zip(places, (5, 4, 4)):
            x, y = nine(dd)
            g = vu.restate(x, y, r, box_of(sim), 1.0)["grains"]        # the restatement first
            assert g["faces"][0] == faces and g["area"][0] == 2.0 ** -18 and g["walls"][0] == 0
            A = upload(sim, x, y)
            R = check(sim, A, 1.0)
            assert R["grains"]["faces"][0] == faces and R["grains"]["area"][0] == 2.0 ** -18
            assert sim.voronoi_grains()["faces"][0] == faces and sim.voronoi_grains()["area"][0] == 2.0 ** -18


@pytest.mark.parametrize("m", [28, 40])
def test_ring_of_neighbours(pkg, m):
    """28 neighbours on a circle: 28 vertices; 40: the cell overflows, with zeros in every measure"""
    th = 2 * np.pi * np.arange(m) / m
    x, y = np.r_[12.8e-3, 12.8e-3 + 8e-3 * np.cos(th)], np.r_[10e-3, 10e-3 + 8e-3 * np.sin(th)]
    r = np.full(m + 1, 0.35e-3)
    with pkg.LbmDem(256, 200, r, x, y) as sim:
        table_substep(sim, None, 1)
        A = restatement_of(sim)
        g = A.at(9e-3)["grains"][0]
        if m == 28:
            assert g["nverts"] == 28 == g["faces"] and g["flags"] == vu.COMPLETE and g["area"] > 0
        else:
            assert g["flags"] == vu.OVERFLOW and A.at(9e-3)["counts"]["overflowed"] == 1
            assert g["nverts"] == g["faces"] == g["walls"] == 0 and g["area"] == g["perimeter"] == g["phi"] == g["R2"] == 0.0
        check(sim, A, 9e-3)
        got = sim.voronoi_grains()[0]
        assert got["nverts"] == g["nverts"] and got["flags"] == g["flags"]


def test_special_centres(pkg):
    """coincident centres, a NaN and two infinite centres, and a grain far outside the box, all in one scene of 65"""
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
            R = check(sim, A, rcut)
            g, c = R["grains"], R["counts"]
            assert c["nonfinite_grains"] == 3 and (g["flags"][[5, 7, 8]] == vu.NONFINITE | vu.EMPTY).all()
            assert (g["nverts"][[5, 7, 8]] == 0).all() and c["empty"] >= 3 and c["overflowed"] == 0
            assert not (g["flags"][20] & (vu.COMPLETE | vu.NONFINITE))
        assert g["nverts"][20] == 4 and g["walls"][20] == 15   # beyond a metre from every grain, the far one has the whole box


def test_small_disc_between_two_large_ones_has_no_cell(pkg):
    r = np.array([0.9e-3, 0.3e-3, 0.9e-3])
    with pkg.LbmDem(256, 200, r, [4e-3, 8e-3, 12e-3], [5e-3, 5e-3, 5e-3]) as sim:
        table_substep(sim, None, 1)
        A = upload(sim, np.array([5e-3, 5.5e-3, 6e-3]), np.array([5e-3, 5e-3, 5e-3]))
        g = A.at(5e-3)["grains"]
        assert g["flags"][1] == vu.EMPTY and g["nverts"][1] == 0 and g["area"][1] == 0.0 and (g["area"][[0, 2]] > 0).all()
        R = check(sim, A, 5e-3)
        assert R["counts"]["empty"] == 1 and R["counts"]["cells"] == 2 and 1 not in R["fsrc"]
        off, src, _ = sim.voronoi_faces()
        assert off[1] == off[2] and 2 in src[off[0]:off[1]] and 0 in src[off[2]:off[3]]


def test_readers_refuse_before_a_compute_and_after_a_move(pkg):
    lx, ly, r, x, y, k = shape_packing(65)
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        calls = (sim.voronoi_grains, sim.voronoi_tensors, sim.voronoi_faces)

        def text(call):
            with pytest.raises(pkg.LbmDemError) as e:
                call()
            assert e.value.code == -1
            return sim._L.lbmdem_last_error().decode()

        def refused():
            for who, call in zip(READERS, calls):
                assert text(call) == NO_COMPUTE % who
        refused()                                   # after create
        assert text(sim.voronoi) == NO_LIST         # no structure compute yet
        table_substep(sim, k, 1)
        refused()
        rcut = 3.3 * 2.0 * float(np.mean(r))
        check(sim, restatement_of(sim), rcut)
        sim.dem_substep()
        refused()                                   # after a sub-step
        assert text(sim.voronoi) == NO_LIST         # the list is stale too
        check(sim, restatement_of(sim), rcut)
        sim.renderScene(1)
        refused()                                   # after a coupled step
        sim.set_diagnostics(True)
        sim.dem_substep()
        check(sim, restatement_of(sim), rcut)
        sim.kinematics = sim.kinematics
        refused()                                   # after an upload of kinematics
        assert text(sim.voronoi) == NO_LIST
        sim.structure(rcut, 7, 1.2, max_entries=0)
        assert text(sim.voronoi) == COUNTS_ONLY     # after a counts-only structure compute
        refused()
        sim.structure(rcut, 7, 1.2)                 # any structure compute with a list will do
        assert sim.voronoi() == restatement_of(sim).at(rcut)["counts"]
        sim.voronoi_faces()                         # reading does not invalidate
        sim.voronoi_grains()
        check(sim, restatement_of(sim), rcut)


def test_refusals(pkg):
    lx, ly, r, x, y, k = shape_packing(65)
    rcut = 2e-3
    if os.path.exists(pkg.SP_LIB_PATH):
        with pkg.LbmDem(lx, ly, r, x, y, precision="f32") as sp:
            for call in (sp.voronoi, sp.voronoi_grains, sp.voronoi_tensors, sp.voronoi_faces, lambda: sp.write_voronoi(".", 0, rcut),
                         lambda: sp.set_voronoi_output(True, rcut)):
                with pytest.raises(pkg.LbmDemError) as e:
                    call()
                assert e.value.code == -1
                assert sp._L.lbmdem_last_error().decode() == "the Voronoi analysis is not available in the single-precision build of the library"

    def text(sim, call):
        with pytest.raises(pkg.LbmDemError) as e:
            call()
        assert e.value.code == -1, e.value
        return sim._L.lbmdem_last_error().decode()
    with pkg.LbmDem(lx, ly, r, x, y, strip=(lx // 2, lx), halo=12) as strip:
        for who, call in (("lbmdem_voronoi_compute", strip.voronoi),
                          ("lbmdem_download_voronoi_grains", strip.voronoi_grains),
                          ("lbmdem_voronoi_grains_device", strip.voronoi_tensors),
                          ("lbmdem_download_voronoi_faces", strip.voronoi_faces),
                          ("lbmdem_voronoi_compute", lambda: strip.write_voronoi(".", 0, rcut)),
                          ("lbmdem_set_voronoi_output", lambda: strip.set_voronoi_output(True, rcut))):
            assert text(strip, call) == who + WHOLE
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert text(sim, lambda: sim.set_voronoi_output(True, bad)).startswith("lbmdem_set_voronoi_output: rcut must be finite and > 0")
        sim.set_voronoi_output(True, rcut)
        assert text(sim, sim.dist_enable) == ("the Voronoi analysis is not available with distributed grains "
                                              "(lbmdem_set_voronoi_output(h, 0, 0.) first)")
        sim.set_voronoi_output(False)
        sim.dist_enable()
        for who, call in (("lbmdem_set_voronoi_output", lambda: sim.set_voronoi_output(True, rcut)),
                          ("lbmdem_voronoi_compute", sim.voronoi),
                          ("lbmdem_voronoi_compute", lambda: sim.write_voronoi(".", 0, rcut))):
            assert text(sim, call) == who + WHOLE


def test_analysis_does_not_interfere(pkg, tmp_path):
    z = np.load(os.path.join(REF_DIR, "inputs_and_table.npz"))
    r, x, y = z["r_mm"] * 1e-3, z["x_mm"] * 1e-3, z["y_mm"] * 1e-3
    rcut = 3.3 * 2.0 * float(r.mean())
    with pkg.LbmDem(256, 200, r, x, y) as a, pkg.LbmDem(256, 200, r, x, y) as b:
        for piece in (1, 7, 3, 13):
            a.renderScene(piece); b.renderScene(piece)
            a.voronoi(rcut); a.voronoi_grains(); a.voronoi_faces(); a.voronoi(rcut / 3)
            a.write_voronoi(str(tmp_path), piece, rcut)
        assert a.nbsteps == b.nbsteps == 24
        for what in ("f", "obst", "kinematics", "fhf"):
            assert np.array_equal(getattr(a, what), getattr(b, what)), what


@pytest.fixture(scope="module")
def g6_scene(pkg, tmp_path_factory):
    """the G6 golden through run_scene to step 4000, with the Voronoi output on and without"""
    z = np.load(os.path.join(REF_DIR, "inputs_and_table.npz"))
    r, x, y = z["r_mm"] * 1e-3, z["x_mm"] * 1e-3, z["y_mm"] * 1e-3
    rcut = 3.3 * 2.0 * float(r.mean())
    with_dir, without_dir = tmp_path_factory.mktemp("with"), tmp_path_factory.mktemp("without")
    with pkg.LbmDem(256, 200, r, x, y) as sim:
        sim.run_scene(4000, str(without_dir))
    with pkg.LbmDem(256, 200, r, x, y) as sim:
        sim.set_voronoi_output(True, rcut)
        sim.run_scene(4000, str(with_dir))
        R = check(sim, restatement_of(sim), rcut)
        c = sim.config()
        got = dict(grains=sim.voronoi_grains(), counts=sim.voronoi(), t=sim.nbsteps * c.dt, W=c.Mdx - c.Mgx, H=c.Mhy - c.Mby)
    return dict(z=z, rcut=rcut, with_dir=with_dir, without_dir=without_dir, R=R, got=got)


def test_g6_at_4000_through_run_scene(pkg, g6_scene, tmp_path):
    S = g6_scene
    new = ["voronoi000000.dat", "voronoi.data"]
    others = sorted(os.listdir(S["without_dir"]))
    assert sorted(os.listdir(S["with_dir"])) == sorted(others + new) and "DEM000000.dat" in others
    for name in others:
        assert (S["with_dir"] / name).read_bytes() == (S["without_dir"] / name).read_bytes(), name
    got = S["got"]
    assert got["counts"] == S["R"]["counts"] and got["counts"]["complete"] > 10 and got["counts"]["grain_faces"] > 100
    pkg.write_voronoi_files(str(tmp_path), 0, got["grains"], S["rcut"], got["counts"], got["t"], got["W"], got["H"])
    for name in new:
        assert (S["with_dir"] / name).read_bytes() == (tmp_path / name).read_bytes(), name
    want = vu.files_text(S["R"]["grains"], S["rcut"], S["R"]["counts"], got["t"], got["W"], got["H"])
    assert (S["with_dir"] / "voronoi000000.dat").read_text() == want[0]
    assert (S["with_dir"] / "voronoi.data").read_text() == vu.DATA_HEADER + want[1]


def test_host_driver_writes_the_voronoi_files(po, g6_scene, tmp_path):
    """`lbmdem <G6> --steps 4001 --voronoi RCUT` in a child process"""
    S, z = g6_scene, g6_scene["z"]
    sample = tmp_path / "packing.data"
    po.write_sample(str(sample), z["r_mm"], z["x_mm"], z["y_mm"])
    out = subprocess.run([EXE, str(sample), "--lx", "256", "--ly", "200", "--steps", "4001", "--voronoi", repr(S["rcut"])],
                         capture_output=True, text=True, cwd=tmp_path, timeout=600)
    assert out.returncode == 0, out.stderr[-600:]
    for name in ("voronoi000000.dat", "voronoi.data"):
        assert (tmp_path / name).read_bytes() == (S["with_dir"] / name).read_bytes(), name
    refused = subprocess.run([EXE, str(sample), "--voronoi", "2e-3", "--gpus", "2"], capture_output=True, text=True, cwd=tmp_path,
                             timeout=120)
    assert refused.returncode != 0 and "--voronoi is a single-GPU mode" in refused.stderr
