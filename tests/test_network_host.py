"""CPU: the pore network's restatement (tests/network_util.py) against a node-by-node loop over the definitions, the identities the
header states, a hand-made dumbbell, the tie rule on a plateau, and lbmdem_write_network_files character for character."""
import os

import numpy as np
import pytest

import clearance_util as cz
import network_util as nu
import pore_util

N = 7
MERGES = (-1, 0, 2)


def test_dtypes_are_the_header_structs(pkg):
    assert nu.NET_BODY_DTYPE == pkg.NET_BODY_DTYPE and nu.NET_BODY_DTYPE.itemsize == 32
    assert nu.NET_GROUP_DTYPE == pkg.NET_GROUP_DTYPE and nu.NET_GROUP_DTYPE.itemsize == 32
    assert nu.NET_LINK_DTYPE == pkg.NET_LINK_DTYPE and nu.NET_LINK_DTYPE.itemsize == 20
    assert nu.NETWORK_COUNTERS == pkg.NETWORK_COUNTERS and len(nu.NETWORK_COUNTERS) == 10


@pytest.mark.parametrize("lx,ly", [(23, 19), (65, 17)])
def test_restatement_equals_the_loop(lx, ly):
    for name, M in cz.shape_maps(lx, ly, N).items():
        for merge in MERGES:
            assert nu.same(nu.restate(M, N, merge), nu.brute_force(M, N, merge)) is None, (name, merge)


def test_identities():
    lx, ly = 65, 17
    for name, M in cz.shape_maps(lx, ly, N).items():
        pores = pore_util.components(M, 8)
        fluid = M == -1
        for merge in MERGES:
            R = nu.restate(M, N, merge)
            c = R["counts"]
            assert int(R["bodies"]["nodes"].sum()) == c["fluid_nodes"] == int(fluid.sum()), name
            assert int(R["groups"]["nodes"].sum()) == c["fluid_nodes"] and int(R["groups"]["bodies"].sum()) == c["bodies"], name
            if merge == -1:
                assert np.array_equal(R["group"], R["body"]) and np.array_equal(R["links0"], R["links1"]), name
                assert c["groups"] == c["bodies"] and c["group_edges"] == c["body_edges"], name
            if name == "all_fluid":
                assert c["bodies"] == 1 and c["body_links"] == 0
            # every conn-8 pore is a union of groups (and so of bodies): a label never spans two pores
            for plane in (R["body"], R["group"]):
                pairs = np.unique(np.stack([plane[fluid], pores[fluid]]), axis=1)
                assert len(np.unique(pairs[0])) == pairs.shape[1], name
            for level in ("links0", "links1"):
                T = R[level]
                assert (T["saddle"] <= R["bodies"]["d2"][T["lo"]]).all() and (T["saddle"] <= R["bodies"]["d2"][T["hi"]]).all(), name
                assert (T["lo"] < T["hi"]).all() and (T["saddle"] >= 1).all()
            assert (R["bodies"]["d2"][R["bodies"]["parent"]] >= R["bodies"]["d2"]).all()
            assert (R["bodies"]["group"][R["bodies"]["group"]] == R["bodies"]["group"]).all()


def test_the_stated_conditions_on_the_gpu_tests_maps():
    maps = cz.shape_maps(127, 121, N)
    c = nu.restate(maps["disc_packing"], N, 1)["counts"]
    assert c["bodies"] >= 2 and c["group_links"] >= 1
    assert nu.restate(maps["checkerboard"], N, 0)["counts"]["groups"] == 1
    assert nu.restate(maps["all_fluid"], N, 0)["counts"]["bodies"] == 1
    R = nu.restate(maps["no_fluid"], N, 0)
    assert R["counts"]["narrowest_saddle"] == -1 and not len(R["bodies"]) and not len(R["groups"]) and not len(R["links1"])


def dumbbell():
    """two squares of 15 x 15 fluid nodes joined by a channel 3 wide and 9 long, in a solid block"""
    M = np.zeros((19, 43), np.int32)
    M[2:17, 2:17] = -1
    M[2:17, 26:41] = -1
    M[8:11, 17:26] = -1
    return M


def test_dumbbell():
    M = dumbbell()
    R = nu.restate(M, N, -1)
    assert R["counts"]["bodies"] == 2 and R["counts"]["body_links"] == 1
    b = R["bodies"]
    # a square of 15: the centre is 8 nodes from the solid; the channel of 3: its middle row is 2 away
    assert list(b["d2"]) == [64, 64] and list(b["node"]) == [9 * 43 + 9, 9 * 43 + 33]
    link = R["links0"][0]
    assert (link["lo"], link["hi"], link["saddle"]) == (0, 1, 4)
    assert link["node"] // 43 == 9 and 17 <= link["node"] % 43 < 26
    assert list(b["degree"]) == [1, 1] and int(b["nodes"].sum()) == 2 * 225 + 27
    # isqrt(64) - isqrt(4) = 6: joined at 6, apart at 5; the smaller index is the higher of two equal peaks
    R5, R6 = nu.restate(M, N, 5), nu.restate(M, N, 6)
    assert R5["counts"]["groups"] == 2 and list(R5["bodies"]["parent"]) == [0, 1]
    assert R6["counts"]["groups"] == 1 and list(R6["bodies"]["parent"]) == [0, 0] and list(R6["bodies"]["group"]) == [0, 0]
    assert R6["counts"]["group_links"] == 0 and R6["counts"]["narrowest_saddle"] == -1 and R6["counts"]["isolated_groups"] == 1
    assert R5["counts"]["narrowest_saddle"] == 4 and R5["counts"]["isolated_groups"] == 0
    for merge in (-1, 5, 6):
        assert nu.same(nu.restate(M, N, merge), nu.brute_force(M, N, merge)) is None


def test_equal_peaks_on_a_plateau_go_to_the_smaller_index():
    """a channel 2 wide: every node has d2 = 1, one plateau; and a channel 4 wide, whose two middle rows tie"""
    M = np.zeros((12, 30), np.int32)
    M[2:4, 1:29] = -1
    M[6:10, 1:29] = -1
    R = nu.restate(M, N, -1)
    assert R["counts"]["bodies"] == 2 and R["counts"]["body_links"] == 0
    assert list(R["bodies"]["node"]) == [2 * 30 + 1, 7 * 30 + 2] and list(R["bodies"]["d2"]) == [1, 4]
    assert (R["body"][2:4, 1:29] == 0).all() and (R["body"][6:10, 1:29] == 1).all()
    assert nu.same(R, nu.brute_force(M, N, -1)) is None


def _args(tmp_path, lx, ly, R, merge, **kw):
    return dict(dict(directory=str(tmp_path), nFile=0, lx=lx, ly=ly, n=N, merge=merge, bodies=R["bodies"], groups=R["groups"],
                     links=R["links1"], counts=R["counts"], t=0.0, body=R["body"], group=R["group"]), **kw)


def test_write_network_files_character_for_character(pkg, tmp_path):
    lx, ly = 65, 17
    for k, (name, merge) in enumerate((("disc_packing", 1), ("random_80", 0), ("no_fluid", -1))):
        R = nu.restate(cz.shape_maps(lx, ly, N)[name], N, merge)
        t = 0.125 + 1e-3 * k
        planes = dict(body=R["body"], group=R["group"]) if k != 1 else dict(body=None, group=None)
        pkg.write_network_files(**_args(tmp_path, lx, ly, R, merge, nFile=k, t=t, **planes))
        want = nu.files_bytes(lx, ly, N, merge, R, t, nfile=k, plane=k != 1)
        data = (tmp_path / "network.data").read_bytes()
        assert data.startswith(nu.DATA_HEADER.encode()) and data.endswith(want.pop("network.data"))
        assert data.count(b"\n") == 2 + k
        for fname, text in want.items():
            assert (tmp_path / fname).read_bytes() == text, fname
        assert os.path.exists(tmp_path / ("network%06d.vtk" % k)) == (k != 1)
        if k == 0:
            assert len(R["links1"]) >= 1 and len(R["groups"]) < len(R["bodies"])
    raw = (tmp_path / "network000000.vtk").read_bytes()
    R0 = nu.restate(cz.shape_maps(lx, ly, N)["disc_packing"], N, 1)
    assert np.array_equal(np.frombuffer(raw[-4 * lx * ly - 1:-1], dtype=">i4").reshape(ly, lx).T, R0["group"])


def test_write_network_files_refusals(pkg, tmp_path):
    lx, ly = 65, 17
    R = nu.restate(cz.shape_maps(lx, ly, N)["random_80"], N, 0)
    assert len(R["links1"]) >= 3 and len(R["groups"]) >= 3 and len(R["groups"]) < len(R["bodies"])

    def text(**kw):
        with pytest.raises(pkg.LbmDemError) as e:
            pkg.write_network_files(**_args(tmp_path, lx, ly, R, 0, **kw))
        assert e.value.code == -1
        return pkg.load_library().lbmdem_last_error().decode()
    assert "cannot open" in text(directory=str(tmp_path / "missing"))
    bad = R["bodies"].copy()
    bad["d2"][2] = -4
    assert text(bodies=bad) == "lbmdem_write_network_files: body 2 has the negative d2 -4"
    bad = R["bodies"].copy()
    bad[[1, 2]] = bad[[2, 1]]
    assert "body 2 has the node" in text(bodies=bad) and "the nodes ascend" in text(bodies=bad)
    merged = int(np.nonzero(R["bodies"]["group"] != np.arange(len(R["bodies"])))[0][0])
    bad = R["bodies"].copy()
    bad["group"][R["groups"]["body"][0]] = merged
    assert text(bodies=bad).endswith("which is not a root")
    bad = R["groups"].copy()
    bad[[1, 2]] = bad[[2, 1]]
    assert "group 2 has the body" in text(groups=bad) and "the bodies ascend" in text(groups=bad)
    bad = R["groups"].copy()          # a body that is not a root, where the table still ascends
    bad["body"][max(int(np.searchsorted(bad["body"], merged)) - 1, 0)] = merged
    assert text(groups=bad).endswith("has the body %d, which is not a root" % merged)
    bad = R["links1"].copy()
    bad[[1, 2]] = bad[[2, 1]]
    assert "link 2 has the pair" in text(links=bad) and "the pairs ascend" in text(links=bad)
    bad = R["links1"].copy()
    bad["lo"][0], bad["hi"][0] = bad["hi"][0], bad["lo"][0]
    assert "link 0 has the pair" in text(links=bad)
    assert "which are not both roots" in text(links=R["links0"]) or "the pairs ascend" in text(links=R["links0"])
    assert os.listdir(tmp_path) == []          # refused before anything is written
    with pytest.raises(pkg.LbmDemError):
        pkg.write_network_files(**_args(tmp_path, lx, ly, R, 0, counts=[0] * 9))
    with pytest.raises(pkg.LbmDemError):
        pkg.write_network_files(**_args(tmp_path, lx, ly, R, 0, group=None))
    with pytest.raises(pkg.LbmDemError):
        pkg.write_network_files(**_args(tmp_path, lx, ly, R, -2))
    # the float library has the formatter too
    if os.path.exists(pkg.SP_LIB_PATH):
        pkg.write_network_files(**_args(tmp_path, lx, ly, R, 0, precision="f32"))
        want = nu.files_bytes(lx, ly, N, 0, R, 0.0, plane=True)
        for fname in ("network_bodies000000.dat", "network_links000000.dat", "network_groups000000.dat", "network000000.vtk"):
            assert (tmp_path / fname).read_bytes() == want[fname], fname
