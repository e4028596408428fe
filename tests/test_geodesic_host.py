"""CPU: the geodesic contract (include/lbmdem_hip.h, "Geodesic") stated twice in tests/geodesic_util.py -- Jacobi sweeps over the
plane and a heap Dijkstra over the grid -- the two against each other, the identities the header names, the conditions the GPU
tests' maps are chosen for, and the host-only formatter character for character."""
import os

import numpy as np
import pytest

import drainage_util as du
import geodesic_util as gu

B, T, L, R = du.SIDE_B, du.SIDE_T, du.SIDE_L, du.SIDE_R
ALL = B | T | L | R
N = 3
PAIRS = ((T, B), (L, R), (ALL, ALL))


def maps():
    out = {"discs %dx%d" % s: du.random_discs(s[0], s[1], N, k) for k, s in enumerate(((13, 61), (33, 62), (64, 64), (127, 121)))}
    out.update(diagonal_passage=du.diagonal_passage(48, 50), two_pores=du.two_pores(48, 50),
               chamber_behind_neck=du.chamber_behind_neck(48, 50), two_routes=du.two_routes(48, 50), serpentine=du.serpentine(),
               comb=gu.comb(48, 50))
    return out


MAPS = maps()


def bfs_steps(P, S):
    """breadth-first steps over the 4-neighbourhood by scipy's masked dilation, -1 where nothing arrives"""
    from scipy import ndimage
    cross = ndimage.generate_binary_structure(2, 1)
    seen = P & S
    steps = np.where(seen, 0, -1)
    k = 0
    while True:
        k += 1
        grown = ndimage.binary_dilation(seen, structure=cross, mask=P)
        new = grown & ~seen
        if not new.any():
            return steps
        steps[new] = k
        seen = grown


@pytest.mark.parametrize("name", list(MAPS))
def test_the_two_statements_agree(name):
    M = MAPS[name]
    lx, ly = M.shape
    band = 4 if name == "serpentine" else 3
    for min_d2 in (0, 4):
        fluid, P = gu.passable(M, N, min_d2)
        for frm, to in PAIRS:
            W = {}
            for conn in (4, 8):
                W[conn] = gu.restate(M, N, frm, band, to, conn, min_d2)
                V = gu.brute_force(M, N, frm, band, to, conn, min_d2)
                assert gu.same(W[conn], V) is None, (name, min_d2, frm, to, conn, gu.same(W[conn], V))
                c, dist, detour = W[conn]["counts"], W[conn]["dist"], W[conn]["detour"]
                assert (detour >= -1).all() and (detour[(dist >= 0) & (W[conn]["back"] >= 0) & (c["shortest"] >= 0)] >= 0).all()
                assert c["path_nodes"] == (detour == 0).sum() and (c["path_nodes"] > 0) == (c["shortest"] >= 0)
                assert W[conn]["profile"]["nodes"].sum() == c["passable_nodes"] == P.sum() and c["fluid_nodes"] == fluid.sum()
                assert W[conn]["profile"]["reached"].sum() == c["reached_nodes"] == (dist >= 0).sum()
                assert (dist[P & du.region(lx, ly, frm, band)] == 0).all() and (dist[~P] == -1).all()
                assert gu.restate(M, N, to, band, frm, conn, min_d2)["counts"]["shortest"] == c["shortest"]
            steps = bfs_steps(P, du.region(lx, ly, frm, band))
            assert np.array_equal(W[4]["dist"], np.where(steps >= 0, gu.AXIS * steps, -1)), (name, min_d2, frm)
            there = W[4]["dist"] >= 0
            assert (W[8]["dist"][there] >= 0).all() and (W[8]["dist"][there] <= W[4]["dist"][there]).all()
            if min_d2:   # a larger min_d2 never lowers a distance
                wide = gu.restate(M, N, frm, band, to, 8, 0)["dist"]
                there = W[8]["dist"] >= 0
                assert (wide[there] >= 0).all() and (wide[there] <= W[8]["dist"][there]).all()
    W = gu.restate(M, N, ALL, max(lx, ly), 0)
    assert (W["dist"][M == -1] == 0).all() and W["counts"]["shortest"] == -1 and (W["back"] == -1).all() and (W["detour"] == -1).all()


def test_the_stated_conditions_on_the_gpu_tests_maps():
    lx, ly = 48, 50
    W = gu.restate(gu.comb(lx, ly), N, B, 1, 0)
    assert W["counts"]["dist_max"] > 5 * 500 and W["counts"]["reached_nodes"] == W["counts"]["passable_nodes"] > 1100
    W = gu.restate(du.serpentine(), N, B, 4, T, 8)
    assert W["counts"]["shortest"] == 5771 > 5000 and W["counts"]["dist_max"] == 5794 and W["counts"]["reached_nodes"] == 6500
    assert gu.restate(du.serpentine(), N, B, 4, T, 4)["counts"]["shortest"] == 6095
    assert gu.restate(du.diagonal_passage(lx, ly), N, B, 4, T, 4)["counts"]["shortest"] == -1
    assert gu.restate(du.diagonal_passage(lx, ly), N, B, 4, T, 8)["counts"]["shortest"] == 217
    assert gu.restate(np.full((lx, ly), -1, np.int32), N, T, 4, B)["counts"]["shortest"] == 215
    c = gu.restate(du.chamber_behind_neck(lx, ly), N, B, 4, 0, 8, 2)["counts"]
    assert (c["reached_nodes"], c["passable_nodes"]) == (139, 380)
    c = gu.restate(du.random_discs(256, 200, 7, 3), 7, T, 4, B)["counts"]
    assert c["outlet_nodes"] > 0 and c["outlet_reached"] == 0 and c["shortest"] == -1
    c = gu.restate(du.two_pores(lx, ly), N, B, 3, T)
    assert (c["dist"][:, ly // 2:] == -1).all() and c["counts"]["shortest"] == -1 and c["counts"]["outlet_nodes"] > 0
    c = gu.restate(du.two_routes(lx, ly), N, B, 4, T)
    assert (c["detour"][6:9, 10] == 0).all() and (c["detour"][lx - 11:lx - 8, 10] == 0).all()


def _args(tmp_path, lx, ly, W, sides, depth, out, steps, least, **kw):
    return dict(dict(directory=str(tmp_path), nFile=0, lx=lx, ly=ly, n=N, frm=sides, band=depth, to=out, conn=steps, min_d2=least,
                     levels=W["profile"], counts=W["counts"], t=0.0, planes=(W["dist"], W["back"], W["detour"])), **kw)


CASES = ((T, 4, B, 8, 0), (L, 3, R, 4, 4), (ALL, 1, ALL, 8, 0))


def test_write_geodesic_files_character_for_character(pkg, tmp_path):
    lx, ly = 40, 45
    for k, (frm, band, to, conn, min_d2) in enumerate(CASES):
        M = du.random_discs(lx, ly, N, k) if k < 2 else np.full((lx, ly), -1, np.int32)
        W = gu.restate(M, N, frm, band, to, conn, min_d2)
        t = 0.125 + 1e-3 * k
        kw = dict(nFile=k, t=t)
        if k == 1:
            kw["planes"] = None
        pkg.write_geodesic_files(**_args(tmp_path, lx, ly, W, frm, band, to, conn, min_d2, **kw))
        want = gu.files_bytes(lx, ly, N, frm, band, to, conn, min_d2, W, t, nfile=k, plane=k != 1)
        data = (tmp_path / "geodesic.data").read_bytes()
        assert data.startswith(gu.DATA_HEADER.encode()) and data.endswith(want.pop("geodesic.data"))
        assert data.count(b"\n") == 2 + k
        for fname, text in want.items():
            assert (tmp_path / fname).read_bytes() == text, fname
        assert os.path.exists(tmp_path / ("geodesic%06d.vtk" % k)) == (k != 1)
    W0 = gu.restate(du.random_discs(lx, ly, N, 0), N, *CASES[0])
    assert W0["counts"]["reached_nodes"] > 0 and (W0["profile"]["reached"][4:] > 0).any()
    raw = (tmp_path / "geodesic000000.vtk").read_bytes()
    assert np.array_equal(np.frombuffer(raw[-4 * lx * ly - 1:-1], dtype=">i4").reshape(ly, lx).T, W0["detour"])
    rows = (tmp_path / "geodesic_profile000000.dat").read_text().splitlines()[2:]
    assert len(rows) == ly and all(r.split()[6] == "0.000000" for r in rows[:4]) and float(rows[10].split()[6]) >= 1.0


def test_write_geodesic_files_refusals(pkg, tmp_path):
    lx, ly = 40, 45
    W = gu.restate(du.random_discs(lx, ly, N, 1), N, T, 4, B)
    assert W["counts"]["reached_nodes"] > 0

    def text(**kw):
        with pytest.raises(pkg.LbmDemError) as e:
            pkg.write_geodesic_files(**_args(tmp_path, kw.pop("lx", lx), ly, W, T, 4, B, 8, 0, **kw))
        assert e.value.code == -1
        return pkg.load_library().lbmdem_last_error().decode()
    assert "cannot open" in text(directory=str(tmp_path / "missing"))
    k = int(np.nonzero(W["profile"]["reached"])[0][0])
    bad = W["profile"].copy()
    bad["reached"][k] = bad["nodes"][k] + 1
    assert text(levels=bad) == ("lbmdem_write_geodesic_files: depth %d has %d nodes, %d reached and the sum %d: 0 <= reached <= nodes, "
                                "0 <= sum" % (k, bad["nodes"][k], bad["reached"][k], bad["sum"][k]))
    bad = W["profile"].copy()
    bad["sum"][k] = -1
    assert "0 <= sum" in text(levels=bad)
    bad = W["profile"].copy()
    bad["dmin"][k] = bad["dmax"][k] + 1
    assert text(levels=bad) == ("lbmdem_write_geodesic_files: depth %d has the least distance %d and the largest %d over %d reached nodes"
                                % (k, bad["dmin"][k], bad["dmax"][k], bad["reached"][k]))
    bad = W["dist"].copy()
    bad[3, 3] = -2
    assert text(planes=(bad, W["back"], W["detour"])) == "lbmdem_write_geodesic_files: dist[3][3] = -2 is below -1"
    assert text(planes=(W["dist"], W["back"], bad)) == "lbmdem_write_geodesic_files: detour[3][3] = -2 is below -1"
    for kw in (dict(frm=0), dict(frm=16), dict(to=-1), dict(to=16), dict(band=0), dict(conn=6), dict(min_d2=-1), dict(levels=W["profile"][:0])):
        assert text(**kw) == "bad lbmdem_write_geodesic_files arguments"
    assert text(lx=1, planes=None) == "lbmdem_write_geodesic_files: the lattice is 1 x 45"
    assert os.listdir(tmp_path) == []          # refused before anything is written
    with pytest.raises(pkg.LbmDemError):
        pkg.write_geodesic_files(**_args(tmp_path, lx, ly, W, T, 4, B, 8, 0, counts=[0] * 9))
    with pytest.raises(pkg.LbmDemError):
        pkg.write_geodesic_files(**_args(tmp_path, lx, ly, W, T, 4, B, 8, 0, planes=(W["dist"], W["back"])))


def test_the_symbols_exist_in_the_library_and_the_python_mirror(pkg):
    names = ("lbmdem_geodesic_compute", "lbmdem_download_geodesic", "lbmdem_geodesic_device", "lbmdem_download_geodesic_profile",
             "lbmdem_geodesic_rounds", "lbmdem_write_geodesic", "lbmdem_set_geodesic_output", "lbmdem_write_geodesic_files")
    declared = pkg.exported_symbols()
    libs = [pkg.load_library()] + ([pkg.load_library("f32")] if os.path.exists(pkg.SP_LIB_PATH) else [])
    for name in names:
        assert name in declared and all(hasattr(lib, name) for lib in libs), name
    for method in ("geodesic", "geodesic_planes", "geodesic_tensors", "geodesic_profile", "geodesic_rounds", "write_geodesic",
                   "set_geodesic_output"):
        assert callable(getattr(pkg.LbmDem, method)), method
    assert pkg.GEODESIC_COUNTERS == gu.GEODESIC_COUNTERS and pkg.GEO_LEVEL_DTYPE == gu.LEVEL_DTYPE and pkg.GEO_UNIT == gu.AXIS
    assert pkg.GEO_LEVEL_DTYPE.itemsize == 32 and callable(pkg.write_geodesic_files)
