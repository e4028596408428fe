"""CPU: the two statements of the pore fluxes (tests/netflux_util.py) -- vectorised numpy and a node-by-node loop in Python
integers -- against each other, the identities the header states, a uniform-velocity equilibrium that pins direction numbering,
opposites and sign to physics, the special values, a hand-set dumbbell, and lbmdem_write_netflux_files character for character."""
import os
import subprocess

import numpy as np
import pytest

import drainage_util as du
import netflux_util as fu
import network_util as nu

N = 7
# D2Q9 as the library numbers it (lbm_device.h: EXq, EYq, Wq)
EX = np.array([0, -1, -1, -1, 0, 1, 1, 1, 0])
EY = np.array([0, 1, 0, -1, -1, -1, 0, 1, 1])
WQ = np.array([4. / 9] + [1. / 36, 1. / 9] * 4)


def random_f(lx, ly, seed):
    return np.random.default_rng(seed).uniform(0.01, 0.5, (lx, ly, 9))


def check_identities(M, f, W, Lp, level, net):
    lx, ly = M.shape
    c = W["counts"]
    assert int(W["regions"]["net_q32"].sum()) == 0
    assert int(W["links"]["edges"].sum()) == c["ridge_edges"] == net["counts"]["group_edges" if level else "body_edges"]
    assert np.array_equal(W["links"]["edges"], W["table"]["edges"])
    assert [fu.wrap(v) for v in Lp["node_net"]] == W["regions"]["net_q32"].tolist()
    col = [0] + W["col"].tolist() + [0]
    row = [0] + W["row"].tolist() + [0]
    assert [fu.wrap(v) for v in Lp["row_in"]] == [fu.wrap(col[x] - col[x + 1]) for x in range(lx)]
    assert [fu.wrap(v) for v in Lp["col_in"]] == [fu.wrap(row[y] - row[y + 1]) for y in range(ly)]
    assert c["fluid_nodes"] == int((M == -1).sum()) and c["regions"] == len(W["regions"]) and c["links"] == len(W["links"])
    assert (W["links"]["exchange_q32"] >= np.abs(W["links"]["flux_q32"])).all()


@pytest.mark.parametrize("lx,ly", [(23, 19), (65, 17)])
def test_the_two_statements_agree_and_the_identities_hold(lx, ly):
    flowing = 0
    for seed in range(2):
        M = du.random_discs(lx, ly, N, 100 * lx + seed)
        f = random_f(lx, ly, seed)
        for merge in (-1, 2):
            net = nu.restate(M, N, merge)
            for level in (0, 1):
                W, Lp = fu.restate(M, f, N, merge, level, N=net), fu.loop(M, f, N, merge, level, N=net)
                assert fu.same(W, Lp) is None, (lx, ly, seed, merge, level, fu.same(W, Lp))
                flowing += W["counts"]["flowing_links"]          # (a small map may be one body, or its groups all merged)
                check_identities(M, f, W, Lp, level, net)
    assert flowing > 0


def test_a_fluid_at_rest_has_no_flux():
    lx, ly = 40, 45
    M = du.random_discs(lx, ly, N, 3)
    f = np.broadcast_to(np.random.default_rng(1).uniform(0.01, 0.5, 9), (lx, ly, 9)).copy()
    # (between two fluid nodes f[q][i] - f[p][opp(i)] compares two directions: equal across the lattice AND i with opp(i))
    f[..., [5, 6, 7, 8]] = f[..., [1, 2, 3, 4]]
    for level in (0, 1):
        W = fu.restate(M, f, N, -1, level)
        c = W["counts"]
        assert not W["col"].any() and not W["row"].any() and not W["links"]["flux_q32"].any() and not W["links"]["exchange_q32"].any()
        assert not W["regions"]["net_q32"].any() and not W["regions"]["through_q32"].any() and W["regions"]["mass_q32"].all()
        assert (c["flowing_links"], c["largest_imbalance"], c["unaccumulated_edges"], c["unaccumulated_nodes"]) == (0, 0, 0, 0)
        assert c["strongest_link"] == (0 if c["links"] else -1) and c["edges"] > 0 and c["ridge_edges"] > 0


def test_a_uniform_velocity_equilibrium_gives_the_darcy_flux():
    """rho = 1, u = (0.01, -0.003) on an all-fluid map: in exact arithmetic the even terms of the equilibrium cancel in
    f_i - f_opp(i), an axis edge carries (2/3) u.e and a diagonal (1/6) u.e. A section towards +x has ly axis edges and 2 (ly - 1)
    diagonal ones whose u_y parts cancel: 2^32 ux (2/3 ly + 2/6 (ly - 1)) = 2^32 ux (ly - 1/3); each edge rounds once (half a unit)
    and its phi carries a few ulp of 0.1: within one unit per edge."""
    lx, ly = 40, 30
    ux, uy = 0.01, -0.003
    eu = EX * ux + EY * uy
    feq = WQ * (1.0 + 3.0 * eu + 4.5 * eu * eu - 1.5 * (ux * ux + uy * uy))
    f = np.broadcast_to(feq, (lx, ly, 9)).copy()
    M = np.full((lx, ly), -1, np.int32)
    for level in (0, 1):
        W = fu.restate(M, f, N, -1, level)
        assert W["counts"]["regions"] == 1 and W["counts"]["links"] == 0 and W["counts"]["strongest_link"] == -1
        assert W["counts"]["edges"] == lx * (ly - 1) + (lx - 1) * ly + 2 * (lx - 1) * (ly - 1)
        want_col, want_row = 2.0 ** 32 * ux * (ly - 1.0 / 3.0), 2.0 ** 32 * uy * (lx - 1.0 / 3.0)
        assert len(W["col"]) == lx - 1 and (np.abs(W["col"] - want_col) <= 3 * ly - 2).all()
        assert len(W["row"]) == ly - 1 and (np.abs(W["row"] - want_row) <= 3 * lx - 2).all()
        assert W["col"].min() > 0 and W["row"].max() < 0          # the sign: towards +x, towards -y
        assert abs(int(W["regions"]["mass_q32"][0]) - lx * ly * 2 ** 32) <= lx * ly * 64
    assert fu.same(fu.restate(M, f, N, -1, 0), fu.loop(M, f, N, -1, 0)) is None


def special_case():
    """an all-fluid 9 x 8 map but one wall column that makes two regions; populations 0.25 with special values at chosen edges"""
    lx, ly = 9, 8
    M = np.full((lx, ly), -1, np.int32)
    M[4, :] = N
    M[4, 3] = -1                                  # a one-node neck
    f = np.full((lx, ly, 9), 0.25)
    k = 12344
    f[1, 2, 8] = 0.25 + (k + 0.5) / 2.0 ** 32     # edge (1,1)->(1,2), direction 8: phi an exact tie, to even
    f[2, 2, 8] = 0.25 + (k + 1.5) / 2.0 ** 32     # ... and the odd neighbour of it
    f[1, 5, 6] = 0.25 + 2.0 ** 20                 # edge (0,5)->(1,5), direction 6: phi == 2^20, left out
    f[1, 6, 6] = 0.25 + 2.0 ** 20 - 2.0 ** -20    # ... just below it: kept
    f[6, 1, 6] = 0.25 - 2.0 ** 20                 # -2^20: left out
    f[6, 5, 7] = np.nan                           # edge (5,4)->(6,5), direction 7, and the node's rho
    f[7, 2, 5] = np.inf                           # edge (6,3)->(7,2), direction 5, and the node's rho
    f[7, 6, 0] = -np.inf                          # a node's rho only: direction 0 is on no edge
    return M, f, k


def test_special_values():
    M, f, k = special_case()
    for level in (0, 1):
        W, Lp = fu.restate(M, f, N, -1, level), fu.loop(M, f, N, -1, level)
        assert fu.same(W, Lp) is None, fu.same(W, Lp)
        c = W["counts"]
        assert c["unaccumulated_edges"] == 4            # 2^20, -2^20, the NaN, the infinity
        # rho: the three nodes with a NaN or an infinity and the two whose rho is above 2^20; -2^20 + 2.25 is kept
        assert c["unaccumulated_nodes"] == 5
    q, out = fu.quantum(np.array([(k + 0.5) / 2.0 ** 32, (k + 1.5) / 2.0 ** 32, 2.0 ** 20, -2.0 ** 20, 2.0 ** 20 - 2.0 ** -20, np.nan, np.inf]))
    assert q.tolist() == [k, k + 2, 0, 0, 2 ** 52 - 2 ** 12, 0, 0] and out.tolist() == [False, False, True, True, False, True, True]
    # (0.25 + x - 0.25 is exact for these x: they are multiples of 2^-33 below 2^21)
    assert W["row"][1] == k + (k + 2)
    assert W["col"][0] == 2 ** 52 - 2 ** 12 and W["col"][5] == 0 and W["col"][6] == 0


def dumbbell():
    """two chambers joined by a channel two nodes wide along x; in the channel one lane flows towards +x, the other towards -x"""
    lx, ly = 21, 11
    M = np.full((lx, ly), N, np.int32)
    M[1:8, 1:10] = -1
    M[13:20, 1:10] = -1
    M[8:13, 5:7] = -1
    f = np.full((lx, ly, 9), 0.125)
    f[8:14, 5, 6] += 3.0 / 2 ** 32          # what arrived going +x along y = 5
    f[7:13, 6, 2] += 5.0 / 2 ** 32          # what arrived going -x along y = 6
    return M, f


def test_a_dumbbell_with_counterflow():
    M, f = dumbbell()
    net = nu.restate(M, N, -1)
    assert net["counts"]["bodies"] >= 2
    for merge in (-1, 0):
        for level in (0, 1):
            W, Lp = fu.restate(M, f, N, merge, level), fu.loop(M, f, N, merge, level)
            assert fu.same(W, Lp) is None
            # every section across the channel carries +3 along y = 5 and -5 along y = 6, whatever the regions are
            assert W["col"][7:13].tolist() == [-2] * 6 and not W["col"][:7].any() and not W["col"][13:].any()
            assert not W["row"].any()
            # the links that cut the channel: counterflow in one throat
            cut = [k for k, e in enumerate(W["links"]) if e["flux_q32"]]
            assert cut and all(W["links"]["flux_q32"][k] in (2, -2) and W["links"]["exchange_q32"][k] == 8 for k in cut)
            assert W["counts"]["flowing_links"] == len(cut) and W["counts"]["strongest_link"] == cut[0]
            assert int(W["regions"]["net_q32"].sum()) == 0 and W["counts"]["largest_imbalance"] == 2
            assert sorted(v for v in W["regions"]["net_q32"].tolist() if v) == [-2, 2]


def _args(tmp_path, lx, ly, W, merge_, level_, **kw):
    merge, level = merge_, level_
    return dict(dict(directory=str(tmp_path), nFile=0, lx=lx, ly=ly, n=N, merge=merge, level=level, links=W["table"], flux=W["links"],
                     region_body=W["region_body"], region_nodes=W["region_nodes"], regions=W["regions"], col=W["col"], row=W["row"],
                     counts=W["counts"], t=0.0), **kw)


def test_write_netflux_files_character_for_character(pkg, tmp_path):
    lx, ly = 40, 45
    for k, (merge, level) in enumerate(((-1, 0), (2, 1), (0, 1))):
        M = du.random_discs(lx, ly, N, k) if k < 2 else np.full((lx, ly), -1, np.int32)
        f = random_f(lx, ly, k) - (0.3 if k == 1 else 0.0)       # (negative numbers in the tables too)
        W = fu.restate(M, f, N, merge, level)
        t = 0.125 + 1e-3 * k
        pkg.write_netflux_files(**_args(tmp_path, lx, ly, W, merge, level, nFile=k, t=t))
        want = fu.files_bytes(lx, ly, N, merge, level, W, t, nfile=k)
        data = (tmp_path / "netflux.data").read_bytes()
        assert data.startswith(fu.DATA_HEADER.encode()) and data.endswith(want.pop("netflux.data"))
        assert data.count(b"\n") == 2 + k
        for fname, text in want.items():
            assert (tmp_path / fname).read_bytes() == text, fname
    assert len(W["links"]) == 0 and len(W["regions"]) == 1          # the last: tables of no link


def test_write_netflux_files_refusals(pkg, tmp_path):
    lx, ly = 40, 45
    M = du.random_discs(lx, ly, N, 1)
    W = fu.restate(M, random_f(lx, ly, 1), N, -1, 0)
    assert len(W["links"]) >= 3 and len(W["regions"]) >= 3

    def text(**kw):
        with pytest.raises(pkg.LbmDemError) as e:
            pkg.write_netflux_files(**_args(tmp_path, lx, ly, W, -1, 0, **kw))
        assert e.value.code == -1
        return pkg.load_library().lbmdem_last_error().decode()
    assert "cannot open" in text(directory=str(tmp_path / "missing"))
    for kw in (dict(merge=-2), dict(level=2), dict(level=-1), dict(n=0)):
        assert text(**kw) == "bad lbmdem_write_netflux_files arguments"
    bad = W["table"].copy()
    bad[[1, 2]] = bad[[2, 1]]
    order = [0, 2, 1] + list(range(3, len(bad)))
    assert "the pairs ascend" in text(links=bad, flux=W["links"][order])
    bad = W["links"].copy()
    bad["edges"][1] += 1
    assert text(flux=bad) == "lbmdem_write_netflux_files: link 1 has %d edges in the network and %d in the fluxes" % (
        W["table"]["edges"][1], W["table"]["edges"][1] + 1)
    bad = W["region_body"].copy()
    bad[2] = bad[1]
    assert "the bodies ascend" in text(region_body=bad)
    bad = W["region_nodes"].copy()
    bad[0] = -1
    assert "a count is not negative" in text(region_nodes=bad)
    assert os.listdir(tmp_path) == []          # refused before anything is written
    for kw in (dict(counts=[0] * 9), dict(col=W["col"][:-1]), dict(row=np.append(W["row"], 0)), dict(flux=W["links"][:-1]),
               dict(regions=W["regions"][:-1])):
        with pytest.raises(pkg.LbmDemError):
            pkg.write_netflux_files(**_args(tmp_path, lx, ly, W, -1, 0, **kw))
    # the float library has the formatter too
    if os.path.exists(pkg.SP_LIB_PATH):
        pkg.write_netflux_files(**_args(tmp_path, lx, ly, W, -1, 0, precision="f32"))
        want = fu.files_bytes(lx, ly, N, -1, 0, W, 0.0)
        for fname in ("netflux_links000000.dat", "netflux_regions000000.dat", "netflux_profile000000.dat"):
            assert (tmp_path / fname).read_bytes() == want[fname], fname


def test_symbols_and_methods_are_there(pkg):
    names = ("lbmdem_netflux_compute lbmdem_download_netflux_links lbmdem_download_netflux_regions lbmdem_download_netflux_profile "
             "lbmdem_write_netflux lbmdem_set_netflux_output lbmdem_write_netflux_files").split()
    for lib in (pkg.LIB_PATH, pkg.SP_LIB_PATH):
        if not os.path.exists(lib):
            continue
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
        assert not [s for s in names if s not in exported], lib
    for method in "netflux netflux_links netflux_regions netflux_profile write_netflux set_netflux_output".split():
        assert callable(getattr(pkg.LbmDem, method)), method
    assert callable(pkg.write_netflux_files) and pkg.NETFLUX_COUNTERS == fu.NETFLUX_COUNTERS and len(pkg.NETFLUX_COUNTERS) == 10
    assert pkg.NETFLUX_LINK_DTYPE == fu.NETFLUX_LINK_DTYPE and pkg.NETFLUX_REGION_DTYPE == fu.NETFLUX_REGION_DTYPE
    assert pkg.NETFLUX_LINK_DTYPE.itemsize == 24 and pkg.NETFLUX_REGION_DTYPE.itemsize == 24
