"""Host only: the numpy restatement of the pore clearance analysis (tests/clearance_util.py) against
scipy.ndimage.distance_transform_edt and a brute-force loop over all pairs, its own identities, and lbmdem_write_clearance_files
character for character against a Python formatter."""
import os

import numpy as np
import pytest

import clearance_util as cz

SHAPES = [(65, 17), (17, 65), (127, 121)]
N = 5
NEW_MAPS = ("sparse_seeds", "far_wall", "two_discs", "owner_ties", "seam_seeds", "disc_packing")


@pytest.mark.parametrize("lx,ly", SHAPES)
def test_d2_is_scipys(lx, ly):
    ndi = pytest.importorskip("scipy.ndimage")
    maps = cz.shape_maps(lx, ly, N)
    assert set(NEW_MAPS) <= set(maps) and len(maps) == 12 + len(NEW_MAPS)
    for name, M in maps.items():
        R = cz.restate(M, N)
        edt = ndi.distance_transform_edt(cz.padded(M, N) == -1)[1:-1, 1:-1]
        assert np.array_equal(R["d2"], np.rint(edt ** 2).astype(np.int64)), name


def brute_throats(d2, owner, fluid, n):
    """the throat table by a Python loop over the nodes"""
    lx, ly = d2.shape
    found = {}
    for x in range(lx):
        for y in range(ly):
            for qx, qy in ((x, y + 1), (x + 1, y)):      # p < q
                if qx >= lx or qy >= ly or not (fluid[x, y] and fluid[qx, qy]) or owner[x, y] == owner[qx, qy]:
                    continue
                pair = (min(owner[x, y], owner[qx, qy]), max(owner[x, y], owner[qx, qy]))
                found.setdefault(pair, []).append((max(d2[x, y], d2[qx, qy]), x * ly + y))
    table = np.zeros(len(found), cz.THROAT_DTYPE)
    for k, pair in enumerate(sorted(found)):
        c, p = min(found[pair])
        table[k] = (pair[0], pair[1], len(found[pair]), c, p)
    return table


def test_against_all_pairs():
    lx, ly = 23, 19
    tied = 0
    for name, M in cz.shape_maps(lx, ly, N).items():
        R = cz.restate(M, N)
        key = cz.brute_force(M, N)
        assert np.array_equal(R["d2"], key >> 32) and np.array_equal(R["owner"], key & 0xFFFFFFFF), name
        table = brute_throats(R["d2"], R["owner"], M == -1, N)
        assert np.array_equal(R["table"], table), name
        if name == "owner_ties":
            # the tie rule decides somewhere: a fluid node with two nearest positions of different owners
            P = cz.padded(M, N)
            sx, sy = np.nonzero(P >= 0)
            for x, y in np.argwhere(M == -1):
                d = (sx - (x + 1)) ** 2 + (sy - (y + 1)) ** 2
                tied += len(np.unique(P[sx, sy][d == d.min()])) > 1
    assert tied >= 4


@pytest.mark.parametrize("lx,ly", SHAPES)
def test_identities(lx, ly):
    for name, M in cz.shape_maps(lx, ly, N).items():
        R = cz.restate(M, N)
        c, t = R["counts"], R["table"]
        fluid = M == -1
        assert R["hist"].sum() == R["owned"].sum() == c["fluid_nodes"] == fluid.sum(), name
        assert t["edges"].sum() == c["ridge_edges"] and len(t) == c["throats"], name
        assert len(R["hist"]) == c["kmax"] + 1 and R["hist"][0] == 0 and (R["hist"][-1] > 0 or c["fluid_nodes"] == 0), name
        assert ((R["d2max"] == -1) == (R["owned"] == 0)).all() and R["d2max"].max() == (c["d2_max"] if c["fluid_nodes"] else -1), name
        assert R["d2"].reshape(-1)[c["d2_max_node"]] == c["d2_max"] and c["sum_d2"] == R["d2"].astype(np.int64).sum(), name
        assert (t["lo"] < t["hi"]).all() and (t["c_min"] >= 1).all() and (t["edges"] >= 1).all(), name
        pairs = t["lo"].astype(np.int64) * (N + 1) + t["hi"]
        assert (np.diff(pairs) > 0).all(), name
        assert c["ownerless_grains"] == int((R["owned"][:N] == 0).sum())
    maps = cz.shape_maps(lx, ly, N)
    empty = cz.restate(maps["no_fluid"], N)["counts"]
    assert empty == dict(zip(cz.CLEARANCE_COUNTERS, (0, 0, 0, 0, 0, 0, 0, -1, N, 0)))
    full = cz.restate(maps["all_fluid"], N)
    half = (min(lx, ly) + 1) // 2
    assert full["counts"]["d2_max"] == half * half and full["counts"]["throats"] == 0 and full["owned"][N] == lx * ly
    assert (full["owner"] == N).all() and full["counts"]["ownerless_grains"] == N
    far = cz.restate(maps["far_wall"], N)
    assert far["d2"][1, ly // 2] == 1 and far["d2"][lx // 2, 0] == 1 and (far["d2"][:, ly // 2] <= (ly // 2 + 1) ** 2).all()


def test_two_discs_have_the_throats_of_their_gaps():
    """two discs of radius 10 whose nearest solid nodes are 6 apart: c_min = (6 / 2)^2; 5 apart: the two middle nodes are 2 from
    either disc"""
    lx, ly = 127, 121
    M = cz.shape_maps(lx, ly, N)["two_discs"]
    t = cz.restate(M, N)["table"]
    by_pair = {(e["lo"], e["hi"]): e for e in t}
    assert by_pair[(0, 1)]["c_min"] == 9 and by_pair[(2, 3)]["c_min"] == 4
    cx = lx // 4
    assert by_pair[(0, 1)]["node"] == cx * ly + 24 and M[cx, 21] == 0 and M[cx, 27] == 1 and (M[cx, 22:27] == -1).all()


def test_write_clearance_files_character_for_character(pkg, tmp_path):
    lx, ly = 65, 17
    for k, name in enumerate(("disc_packing", "random_40", "no_fluid")):
        R = cz.restate(cz.shape_maps(lx, ly, N)[name], N)
        t = 0.125 + 1e-3 * k
        planes = dict(d2=R["d2"], owner=R["owner"]) if k != 1 else {}
        pkg.write_clearance_files(str(tmp_path), k, lx, ly, R["table"], R["hist"], R["owned"], R["d2max"], R["counts"], t, **planes)
        want = cz.files_bytes(lx, ly, N, R, t, nfile=k, plane=k != 1)
        data = (tmp_path / "clearance.data").read_bytes()
        assert data.startswith(cz.DATA_HEADER.encode()) and data.endswith(want.pop("clearance.data"))
        assert data.count(b"\n") == 2 + k
        for fname, text in want.items():
            assert (tmp_path / fname).read_bytes() == text, fname
        assert os.path.exists(tmp_path / ("clearance%06d.vtk" % k)) == (k != 1)
    # the planes, read back
    raw = (tmp_path / "clearance000000.vtk").read_bytes()
    R0 = cz.restate(cz.shape_maps(lx, ly, N)["disc_packing"], N)
    at = raw.index(b"SCALARS d2 int 1\nLOOKUP_TABLE default\n") + len(b"SCALARS d2 int 1\nLOOKUP_TABLE default\n")
    assert np.array_equal(np.frombuffer(raw[at:at + 4 * lx * ly], dtype=">i4").reshape(ly, lx).T, R0["d2"])
    assert np.array_equal(np.frombuffer(raw[-4 * lx * ly - 1:-1], dtype=">i4").reshape(ly, lx).T, R0["owner"])


def test_write_clearance_files_refusals(pkg, tmp_path):
    lx, ly = 65, 17
    R = cz.restate(cz.shape_maps(lx, ly, N)["disc_packing"], N)
    assert len(R["table"]) >= 3
    args = lambda **kw: dict(dict(directory=str(tmp_path), nFile=0, lx=lx, ly=ly, table=R["table"], hist=R["hist"], owned=R["owned"],
                                  d2max=R["d2max"], counts=R["counts"], t=0.0, d2=R["d2"], owner=R["owner"]), **kw)

    def text(**kw):
        with pytest.raises(pkg.LbmDemError) as e:
            pkg.write_clearance_files(**args(**kw))
        assert e.value.code == -1
        return pkg.load_library().lbmdem_last_error().decode()
    assert "cannot open" in text(directory=str(tmp_path / "missing"))
    bad = R["d2"].copy()
    bad[3, 4] = -1
    assert text(d2=bad) == "lbmdem_write_clearance_files: d2[3][4] = -1 is negative"
    bad = R["owner"].copy()
    bad[3, 4] = N + 1
    assert text(owner=bad) == "lbmdem_write_clearance_files: owner[3][4] = %d is outside [0, %d]" % (N + 1, N)
    bad[3, 4] = -1
    assert "owner[3][4] = -1" in text(owner=bad)
    swapped = R["table"].copy()
    swapped[[1, 2]] = swapped[[2, 1]]
    assert "entry 2 of the table" in text(table=swapped) and "the pairs ascend" in text(table=swapped)
    assert os.listdir(tmp_path) == []          # refused before anything is written
    with pytest.raises(pkg.LbmDemError):
        pkg.write_clearance_files(**args(counts=[0] * 9))
    with pytest.raises(pkg.LbmDemError):
        pkg.write_clearance_files(**args(owner=None))
    # the float library has the formatter too
    if os.path.exists(pkg.SP_LIB_PATH):
        pkg.write_clearance_files(**args(precision="f32"))
        want = cz.files_bytes(lx, ly, N, R, 0.0, plane=True)
        assert (tmp_path / "throats000000.dat").read_bytes() == want["throats000000.dat"]
