"""Host only: the numpy restatement of the pore space analysis (tests/pore_util.py) against scipy.ndimage.label, its own
invariants, and lbmdem_write_pore_files character for character against a Python formatter."""
import os

import numpy as np
import pytest

import packing_util as pu
import pore_util as pz

SHAPES = [(65, 17), (17, 65), (127, 121)]
N = 5


def some_f(lx, ly, seed=3):
    """populations around the rest state, every node different; one NaN, one infinity, one beyond 2^20"""
    rng = np.random.default_rng(seed)
    w = np.array([4 / 9] + [1 / 36, 1 / 9] * 4)
    f = w * (1.0 + 0.05 * rng.standard_normal((lx, ly, 9)))
    f[lx // 2, ly // 2, 3] = np.nan
    f[lx // 3, ly // 3, 0] = np.inf
    f[2, 2, 1] = 2.0 ** 21
    return f


def same_partition(a, b):
    """two labellings of the same nodes name the same sets"""
    pairs = np.unique(np.stack([a, b], axis=1), axis=0)
    return len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1]))


@pytest.mark.parametrize("lx,ly", SHAPES)
def test_partition_is_scipys(lx, ly):
    ndi = pytest.importorskip("scipy.ndimage")
    for name, M in pz.shape_maps(lx, ly, N).items():
        fluid = M == -1
        for conn, structure in ((4, [[0, 1, 0], [1, 1, 1], [0, 1, 0]]), (8, np.ones((3, 3), int))):
            label = pz.components(M, conn)
            ref, count = ndi.label(fluid, structure=structure)
            assert ((label >= 0) == fluid).all(), name
            assert len(np.unique(label[fluid])) == count, (name, conn)
            assert same_partition(label[fluid], ref[fluid]), (name, conn)


@pytest.mark.parametrize("lx,ly", SHAPES)
def test_labels_are_minima_and_the_table_adds_up(lx, ly):
    f = some_f(lx, ly)
    idx = np.arange(lx * ly).reshape(lx, ly)
    for name, M in pz.shape_maps(lx, ly, N).items():
        for conn in (4, 8):
            R = pz.restate(M, f, N, conn)
            label, table, c = R["label"], R["table"], R["counts"]
            fluid = M == -1
            # a label is a node of its own component, and no node of the component is smaller
            assert (label[fluid] <= idx[fluid]).all() and (label.reshape(-1)[label[fluid]] == label[fluid]).all(), name
            assert (np.diff(table["label"]) > 0).all() and table["nodes"].sum() == fluid.sum() == c["fluid_nodes"], name
            assert c["components"] == len(table) and c["trapped_nodes"] == c["fluid_nodes"] - c["largest_nodes"]
            assert (table["grain_links"] + table["wall_links"] <= 8 * table["nodes"]).all()
            assert ((R["pore_min"] == -1) == (R["wet"] == 0)).all() and (R["pore_min"] <= R["pore_max"]).all()
            assert R["wet"].sum() == table["grain_links"].sum()     # every wetted link is seen from both sides
            assert c["unaccumulated"] == int((fluid & ~(np.abs(pz.rho_of(f)) < 2.0 ** 20)).sum())
    half = (lx * ly + 1) // 2
    c4 = pz.restate(pz.shape_maps(lx, ly, N)["checkerboard"], f, N, 4)["counts"]
    c8 = pz.restate(pz.shape_maps(lx, ly, N)["checkerboard"], f, N, 8)["counts"]
    assert c4["components"] == c4["single_nodes"] == half and c8["components"] == 1 and c8["largest_nodes"] == half
    maps = pz.shape_maps(lx, ly, N)
    assert pz.restate(maps["antidiagonal_stripes"], f, N, 4)["counts"]["single_nodes"] > lx * ly // 4
    assert pz.restate(maps["antidiagonal_stripes"], f, N, 8)["counts"]["single_nodes"] <= 2
    for name in ("serpentine", "comb", "u_shape", "all_fluid"):
        assert pz.restate(maps[name], f, N, 4)["counts"]["components"] == 1, name
    assert pz.restate(maps["serpentine"], f, N, 4)["counts"]["largest_nodes"] > lx * ly // 2
    assert pz.restate(maps["spiral"], f, N, 4)["counts"]["largest_nodes"] > lx * ly // 3
    assert pz.restate(maps["all_fluid"], f, N, 8)["counts"]["spanning"] == 3
    assert pz.restate(maps["no_fluid"], f, N, 8)["counts"]["largest_label"] == -1
    assert pz.restate(maps["one_node"], f, N, 8)["table"]["label"][0] == (lx // 2) * ly + ly - 1


def pocket_scene():
    """a dense triangular packing of touching discs: rasterised with the full radius (reductionR = 1) the gaps between three
    discs are sealed pockets"""
    lx, ly = 127, 121
    r, x, y = pu.tri_packing_m(lx, ly, 0.6)
    return lx, ly, r, x, y


def test_the_pocket_scene_has_pockets(po):
    lx, ly, r, x, y = pocket_scene()
    ora = po.Oracle(lx, ly, r, x, y)
    ora.set_reduction(1.0)
    M = ora.get_obst()
    f = np.ones((lx, ly, 9)) / 9
    for conn in (4, 8):
        R = pz.restate(M, f, len(r), conn)
        assert R["counts"]["components"] > 1 and R["counts"]["trapped_nodes"] > 0, R["counts"]
        assert R["counts"]["throat_grains"] > 0 and (R["pore_min"] != R["pore_max"]).any()


def test_write_pore_files_character_for_character(pkg, tmp_path):
    lx, ly = 65, 17
    f = some_f(lx, ly)
    for k, (name, conn) in enumerate((("random_60", 4), ("random_40", 8), ("no_fluid", 8))):
        R = pz.restate(pz.shape_maps(lx, ly, N)[name], f, N, conn)
        t = 0.125 + 1e-3 * k
        pkg.write_pore_files(str(tmp_path), k, conn, lx, ly, R["table"], R["wet"], R["pore_min"], R["pore_max"], R["counts"], t,
                             label=R["label"] if k != 1 else None)
        want = pz.files_bytes(conn, lx, ly, R, t, nfile=k, plane=k != 1)
        data = (tmp_path / "pores.data").read_bytes()
        assert data.startswith(pz.DATA_HEADER.encode()) and data.endswith(want.pop("pores.data"))
        assert data.count(b"\n") == 2 + k
        for fname, text in want.items():
            assert (tmp_path / fname).read_bytes() == text, fname
        assert os.path.exists(tmp_path / ("pores%06d.vtk" % k)) == (k != 1)
    # the plane, read back
    raw = (tmp_path / "pores000000.vtk").read_bytes()
    body = np.frombuffer(raw[-4 * lx * ly:], dtype=">i4").reshape(ly, lx)
    R0 = pz.restate(pz.shape_maps(lx, ly, N)["random_60"], f, N, 4)
    assert np.array_equal(body.T, R0["label"]) and b"SCALARS pore int 1\nLOOKUP_TABLE default\n" in raw[:400]
    back = np.fromfile(tmp_path / "pores000000.vtk", dtype=">i4", offset=len(raw) - 4 * lx * ly)
    assert np.array_equal(back.reshape(ly, lx).T, R0["label"])


def test_write_pore_files_refusals(pkg, tmp_path):
    lx, ly = 65, 17
    R = pz.restate(pz.shape_maps(lx, ly, N)["random_60"], some_f(lx, ly), N, 8)
    args = lambda **kw: dict(dict(directory=str(tmp_path), nFile=0, conn=8, lx=lx, ly=ly, table=R["table"], wet=R["wet"],
                                  pore_min=R["pore_min"], pore_max=R["pore_max"], counts=R["counts"], t=0.0, label=R["label"]), **kw)

    def text(**kw):
        with pytest.raises(pkg.LbmDemError) as e:
            pkg.write_pore_files(**args(**kw))
        assert e.value.code == -1
        return pkg.load_library().lbmdem_last_error().decode()
    assert "cannot open" in text(directory=str(tmp_path / "missing"))
    assert text(conn=6) == "lbmdem_write_pore_files: conn is 4 or 8 (6)"
    bad = R["label"].copy()
    bad[3, 4] = lx * ly
    assert text(label=bad) == "lbmdem_write_pore_files: label[3][4] = %d is outside [-1, %d)" % (lx * ly, lx * ly)
    bad[3, 4] = -2
    assert "label[3][4] = -2" in text(label=bad)
    swapped = R["table"].copy()
    swapped[[1, 2]] = swapped[[2, 1]]
    assert "entry 2 of the table" in text(table=swapped) and "the labels ascend" in text(table=swapped)
    assert os.listdir(tmp_path) == []          # refused before anything is written
    with pytest.raises(pkg.LbmDemError):
        pkg.write_pore_files(**args(counts=[0] * 9))
    # the float library has the formatter too
    if os.path.exists(pkg.SP_LIB_PATH):
        pkg.write_pore_files(**args(precision="f32"))
        want = pz.files_bytes(8, lx, ly, R, 0.0, plane=True)
        assert (tmp_path / "pore_table000000.dat").read_bytes() == want["pore_table000000.dat"]
