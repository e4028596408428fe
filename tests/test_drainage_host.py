"""CPU: the two statements of drainage (tests/drainage_util.py) -- the relaxation over the pore network and a heap-based widest
path over the grid -- against each other, the identities the header states, the conditions the GPU tests' maps are chosen for,
and lbmdem_write_drainage_files character for character."""
import os
import subprocess

import numpy as np
import pytest

import clearance_util as cz
import drainage_util as du
import network_util as nu
import pore_util

N = 7
B, T, L, R = du.SIDE_B, du.SIDE_T, du.SIDE_L, du.SIDE_R
ALL = B | T | L | R
CASES = ((T, 4, B), (L, 3, R), (ALL, 1, ALL), (B, 2, 0), (R | T, 6, L))
SHAPES = [(13, 61), (33, 62), (40, 45), (64, 64)]


def agree(M, frm, band, to, what, net=None):
    W, F = du.restate(M, N, frm, band, to, N=net), du.brute_force(M, N, frm, band, to)
    assert np.array_equal(W["access"], F["access"]), (what, frm, band, to)
    assert np.array_equal(W["hist"], F["hist"]), (what, frm, band, to)
    assert {k: W["counts"][k] for k in du.NODE_COUNTERS} == F["counts"], (what, frm, band, to)
    return W


@pytest.mark.parametrize("lx,ly", SHAPES)
def test_the_two_statements_agree(lx, ly):
    for seed in range(3):
        M = du.random_discs(lx, ly, N, 100 * lx + seed)
        net = nu.restate(M, N, -1)
        for frm, band, to in CASES:
            agree(M, frm, band, to, (lx, ly, seed), net)


def test_the_two_statements_agree_on_the_hand_made_maps():
    for name, M in (("two_pores", du.two_pores(41, 47)), ("chamber", du.chamber_behind_neck(45, 43)), ("diagonal", du.diagonal_passage(41, 44)),
                    ("two_routes", du.two_routes(48, 50)), ("serpentine", du.serpentine())):
        net = nu.restate(M, N, -1)
        for frm, band, to in CASES[:3]:
            agree(M, frm, band, to, name, net)


def test_identities():
    lx, ly = 40, 45
    for seed in range(4):
        M = du.random_discs(lx, ly, N, seed)
        net = nu.restate(M, N, -1)
        d2, body, fluid = net["d2"], net["body"], M == -1
        pores = pore_util.components(M, 8)
        for frm, band, to in CASES:
            W = du.restate(M, N, frm, band, to, N=net)
            c = W["counts"]
            assert int(W["hist"].sum()) == c["fluid_nodes"] and W["hist"][0] == c["fluid_nodes"] - c["reached_nodes"]
            assert (W["access"] <= d2).all() and c["critical"] <= c["access_max"]
            S = fluid & du.region(lx, ly, frm, band)
            assert np.array_equal(W["access"][S], d2[S])
            top = np.zeros(len(W["A"]), np.int64)          # A is the largest access of the body's nodes
            np.maximum.at(top, body[fluid], W["access"][fluid])
            assert np.array_equal(top, W["A"]) and (W["A"] <= net["bodies"]["d2"]).all()
            with_inlet = np.unique(pores[S])
            assert not W["access"][fluid & ~np.isin(pores, with_inlet)].any()
            assert (W["access"][fluid & np.isin(pores, with_inlet)] > 0).all()
            assert len(W["hist"]) == len(cz.restate(M, N)["hist"])
            if to:
                assert du.restate(M, N, to, band, frm, N=net)["counts"]["critical"] == c["critical"]
        W = du.restate(M, N, ALL, max(lx, ly), 0, N=net)
        assert np.array_equal(W["access"], d2) and W["counts"]["critical"] == -1 and W["counts"]["shielded_nodes"] == 0


def test_the_stated_conditions_on_the_gpu_tests_maps():
    lx, ly = 48, 50
    W = du.restate(du.two_pores(lx, ly), N, B, 3, T)
    assert (W["access"][:, ly // 2:] == 0).all() and W["hist"][0] > 0 and W["counts"]["critical"] == 0
    W = du.restate(du.chamber_behind_neck(lx, ly), N, B, 4, 0)
    assert (W["access"][lx // 2 - 8:lx // 2 + 9, 11:29] == 1).all() and W["counts"]["shielded_nodes"] >= 17 * 18 - 100
    assert W["network"]["d2"][lx // 2, 20] > 1
    W = du.restate(du.diagonal_passage(lx, ly), N, B, 4, T)
    assert W["counts"]["critical"] == 1 and W["counts"]["front_links"] >= 1
    W = du.restate(du.two_routes(lx, ly), N, B, 4, T)
    assert W["counts"]["critical"] == 4 and W["counts"]["front_links"] == 2
    W = du.restate(du.serpentine(), N, B, 4, T)
    assert len(W["passes"]) > 256 and W["rounds"] > 100 and W["counts"]["critical"] >= 1
    assert W["counts"]["reached_nodes"] == W["counts"]["fluid_nodes"]


def _args(tmp_path, lx, ly, W, chist, sides, depth, out, **kw):
    return dict(dict(directory=str(tmp_path), nFile=0, lx=lx, ly=ly, n=N, frm=sides, band=depth, to=out, bodies=W["network"]["bodies"],
                     A=W["A"], hist=W["hist"], clearance_hist=chist, counts=W["counts"], t=0.0, access=W["access"]), **kw)


def test_write_drainage_files_character_for_character(pkg, tmp_path):
    lx, ly = 40, 45
    for k, (frm, band, to) in enumerate(CASES[:3]):
        M = du.random_discs(lx, ly, N, k) if k < 2 else np.zeros((lx, ly), np.int32)
        W, chist = du.restate(M, N, frm, band, to), cz.restate(M, N)["hist"]
        t = 0.125 + 1e-3 * k
        pkg.write_drainage_files(**_args(tmp_path, lx, ly, W, chist, frm, band, to, nFile=k, t=t, access=W["access"] if k != 1 else None))
        want = du.files_bytes(lx, ly, N, frm, band, to, W, chist, t, nfile=k, plane=k != 1)
        data = (tmp_path / "drainage.data").read_bytes()
        assert data.startswith(du.DATA_HEADER.encode()) and data.endswith(want.pop("drainage.data"))
        assert data.count(b"\n") == 2 + k
        for fname, text in want.items():
            assert (tmp_path / fname).read_bytes() == text, fname
        assert os.path.exists(tmp_path / ("drainage%06d.vtk" % k)) == (k != 1)
    raw = (tmp_path / "drainage000000.vtk").read_bytes()
    W0 = du.restate(du.random_discs(lx, ly, N, 0), N, *CASES[0])
    assert W0["access"].any()
    assert np.array_equal(np.frombuffer(raw[-4 * lx * ly - 1:-1], dtype=">i4").reshape(ly, lx).T, W0["access"])


def test_write_drainage_files_refusals(pkg, tmp_path):
    lx, ly = 40, 45
    M = du.random_discs(lx, ly, N, 1)
    W, chist = du.restate(M, N, T, 4, B), cz.restate(M, N)["hist"]
    assert len(W["A"]) >= 3 and W["A"].max() > 0

    def text(**kw):
        with pytest.raises(pkg.LbmDemError) as e:
            pkg.write_drainage_files(**_args(tmp_path, lx, ly, W, chist, T, 4, B, **kw))
        assert e.value.code == -1
        return pkg.load_library().lbmdem_last_error().decode()
    assert "cannot open" in text(directory=str(tmp_path / "missing"))
    bad = W["A"].copy()
    bad[1] = W["network"]["bodies"]["d2"][1] + 1
    assert text(A=bad) == "lbmdem_write_drainage_files: body 1 has A = %d above its d2 = %d" % (bad[1], bad[1] - 1)
    bad = W["A"].copy()
    bad[2] = -3
    assert text(A=bad) == "lbmdem_write_drainage_files: body 2 has the negative A -3"
    assert text(A=W["A"][:-1]) == "lbmdem_write_drainage_files: there are %d bodies and %d values of A" % (len(W["A"]), len(W["A"]) - 1)
    assert text(hist=W["hist"][:-1]) == ("lbmdem_write_drainage_files: the access histogram has %d bins, the clearance histogram %d"
                                         % (len(chist) - 1, len(chist)))
    bad = W["hist"].copy()
    bad[0] = -1
    assert "a count is not negative" in text(hist=bad)
    bad = W["network"]["bodies"].copy()
    bad[[1, 2]] = bad[[2, 1]]
    assert "the nodes ascend" in text(bodies=bad, A=W["A"][[0, 2, 1] + list(range(3, len(W["A"])))])
    bad = W["access"].copy()
    bad[3, 3] = -1
    assert text(access=bad) == "lbmdem_write_drainage_files: access[3][3] = -1 is negative"
    for kw in (dict(frm=0), dict(frm=16), dict(to=-1), dict(to=16), dict(band=0)):
        assert text(**kw) == "bad lbmdem_write_drainage_files arguments"
    assert os.listdir(tmp_path) == []          # refused before anything is written
    with pytest.raises(pkg.LbmDemError):
        pkg.write_drainage_files(**_args(tmp_path, lx, ly, W, chist, T, 4, B, counts=[0] * 9))
    with pytest.raises(pkg.LbmDemError):
        pkg.write_drainage_files(**_args(tmp_path, lx, ly, W, chist, T, 4, B, access=W["access"].T))
    # the float library has the formatter too
    if os.path.exists(pkg.SP_LIB_PATH):
        pkg.write_drainage_files(**_args(tmp_path, lx, ly, W, chist, T, 4, B, precision="f32"))
        want = du.files_bytes(lx, ly, N, T, 4, B, W, chist, 0.0, plane=True)
        for fname in ("drainage_curve000000.dat", "drainage_bodies000000.dat", "drainage000000.vtk"):
            assert (tmp_path / fname).read_bytes() == want[fname], fname


def test_symbols_and_methods_are_there(pkg):
    names = ("lbmdem_drainage_compute lbmdem_download_drainage lbmdem_drainage_device lbmdem_download_drainage_bodies "
             "lbmdem_download_drainage_links lbmdem_download_drainage_hist lbmdem_drainage_rounds lbmdem_write_drainage "
             "lbmdem_set_drainage_output lbmdem_write_drainage_files").split()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [s for s in names if s not in exported]
    for method in ("drainage drainage_plane drainage_tensor drainage_bodies drainage_links drainage_hist drainage_rounds write_drainage "
                   "set_drainage_output").split():
        assert callable(getattr(pkg.LbmDem, method)), method
    assert callable(pkg.write_drainage_files) and pkg.DRAINAGE_COUNTERS == du.DRAINAGE_COUNTERS and len(pkg.DRAINAGE_COUNTERS) == 10
    assert (pkg.SIDE_B, pkg.SIDE_T, pkg.SIDE_L, pkg.SIDE_R) == (1, 2, 4, 8)
