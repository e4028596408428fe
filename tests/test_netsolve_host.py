"""CPU: the restatement of the network pressures (tests/netsolve_util.py) pinned, so that the GPU tests may trust it -- against
numpy.linalg.solve on the dense matrix of the free regions, the exact identities the header states, the stop rules, and
lbmdem_write_netsolve_files character for character with every refusal."""
import os
import subprocess

import numpy as np
import pytest

import drainage_util as du
import netsolve_util as su
import network_util as nu

N = 7
B, T, L, R = du.SIDE_B, du.SIDE_T, du.SIDE_L, du.SIDE_R


def against_the_direct_solve(M, frm, band, to, merge, level, model, seed=0):
    """the bound of the issue: |x - x*|_2 <= cond_2(A) * (rho + R * 2^-52) * |x*|_2, rho the true relative residual of x in numpy,
    the second term the direct solve's own backward error -> (rho, cond, iterations, free regions solved for)"""
    net = nu.restate(M, N, merge)
    g = None
    if model == 1:
        g = np.random.default_rng(seed).uniform(0.05, 3.0, len(net["links1" if level else "links0"]))
    W = su.restate(M, N, frm, band, to, merge, level, model=model, g_user=g, rtol=1e-10, max_iter=su.AUTO_CAP, N=net)
    assert W["counts"]["status"] == 0, W["counts"]          # (a chain of regions in series may need more than one iteration each)
    A, rhs, f = su.dense(W)
    loose = W["free"] & ~su.anchored(W)
    assert not W["x"][loose].any() and not W["x"][~W["free"]].any()
    if len(f) == 0:
        return 0.0, 1.0, W["counts"]["iterations"], 0
    assert np.array_equal(A, A.T) and np.allclose(rhs, W["b"][f], rtol=1e-13, atol=0.0)
    x = W["x"][f]
    xs = np.linalg.solve(A, rhs)
    rho = float(np.linalg.norm(rhs - A @ x) / np.linalg.norm(rhs)) if rhs.any() else 0.0
    cond = float(np.linalg.cond(A))
    err, bound = float(np.linalg.norm(x - xs)), cond * (rho + len(W["regions"]) * 2.0 ** -52) * float(np.linalg.norm(xs))
    print("rho %.3e cond %.3e iterations %d free %d err %.3e bound %.3e" % (rho, cond, W["counts"]["iterations"], len(f), err, bound))
    assert err <= bound, (err, bound, rho, cond)
    assert ((xs > -1e-9) & (xs < 1 + 1e-9)).all()          # the maximum principle
    return rho, cond, W["counts"]["iterations"], len(f)


@pytest.mark.parametrize("lx,ly", [(64, 64), (127, 121)])
@pytest.mark.parametrize("model", [0, 1])
def test_rasterised_packings_against_the_direct_solve(lx, ly, model):
    solved = 0
    for seed in range(2):
        M = du.random_discs(lx, ly, N, 100 * lx + seed)
        for merge, level in ((-1, 0), (1, 1)):
            for frm, band, to in ((T, 4, B), (L, 3, R)):
                solved += against_the_direct_solve(M, frm, band, to, merge, level, model, seed)[3]
    assert solved > 0


@pytest.mark.parametrize("model", [0, 1])
def test_callers_maps_against_the_direct_solve(model):
    lx, ly = 48, 50
    solved = 0
    for M in (du.chamber_behind_neck(lx, ly), du.two_routes(lx, ly), du.serpentine(), su.star(), su.chambers(61, 46)):
        solved += against_the_direct_solve(M, B, 5, T, -1, 0, model)[3]
    assert solved > 0


def test_two_pores_keep_exact_zeros_behind_the_wall():
    lx, ly = 48, 50
    M = du.two_pores(lx, ly)
    for level in (0, 1):
        W = su.restate(M, N, B, 3, L | R, 0, level)
        c = W["counts"]
        assert c["inlet_regions"] >= 1 and c["regions"] >= 2
        # the regions of the pore at high y: no inlet in their component
        reg = su.regions_of(nu.restate(M, N, 0), level)[0]
        far = np.unique(reg[:, ly // 2 + 2:][reg[:, ly // 2 + 2:] >= 0])
        assert len(far) >= 1 and not W["regions"]["p"][far].view(np.int64).any()       # +0.0 on the bits
        touching = np.isin(W["lo"], far) | np.isin(W["hi"], far)
        assert not W["links"]["q"][touching].view(np.int64).any()
        fixed = W["regions"]["flags"] != 0
        assert set(W["regions"]["p"][fixed].tolist()) <= {0.0, 1.0}


def test_an_inlet_band_without_fluid_is_no_error():
    lx, ly = 48, 50
    M = du.random_discs(lx, ly, N, 5)
    M[:, :3] = N
    W = su.restate(M, N, B, 3, T, -1, 0)
    c = W["counts"]
    assert c["inlet_regions"] == 0 and c["iterations"] == 0 and c["status"] == 0 and c["flowing_links"] == 0 and c["outlet_regions"] >= 1
    assert not W["regions"]["p"].any() and not W["links"]["q"].any() and W["sums"] == dict(Q_in=0.0, Q_out=0.0, rz0=0.0, rz=0.0)
    assert c["strongest_link"] == (0 if c["links"] else -1)


def test_from_equal_to_shorts_every_fixed_region():
    M = du.random_discs(64, 64, N, 2)
    W = su.restate(M, N, T, 4, T, -1, 0)
    c = W["counts"]
    assert c["inlet_regions"] == c["shorted_regions"] >= 1 and c["outlet_regions"] == 0
    fixed = W["regions"]["flags"] != 0
    assert (W["regions"]["flags"][fixed] == 5).all() and (W["regions"]["p"][fixed] == 1.0).all()
    # nothing is held at 0: every anchored region ends at 1
    assert np.allclose(W["regions"]["p"][su.anchored(W)], 1.0, atol=1e-6)


def test_an_all_fluid_map_is_one_shorted_region():
    M = np.full((48, 50), -1, np.int32)
    for level in (0, 1):
        W = su.restate(M, N, B, 2, T, -1, level)
        assert W["counts"] == dict(zip(su.NETSOLVE_COUNTERS, (1, 0, 1, 0, 1, 0, 0, 0, 0, -1)))
        assert W["regions"]["p"].tolist() == [1.0] and W["regions"]["net"].tolist() == [0.0] and W["regions"]["flags"].tolist() == [5]
    W = su.restate(np.full((48, 50), N, np.int32), N, B, 2, T, -1, 0)          # no fluid at all: no region
    assert W["counts"] == dict(zip(su.NETSOLVE_COUNTERS, (0, 0, 0, 0, 0, 0, 0, 0, 0, -1)))


def test_two_routes_carry_the_same_flow_on_the_bits():
    """two channels of the same shape between the reservoir and the chamber: the same saddle and the same distance between the
    peaks on either side, so the same g, and the same q on the bits"""
    W = su.restate(du.two_routes(48, 50), N, B, 3, T, -1, 0)
    q = W["links"]["q"][W["links"]["q"] != 0]
    assert len(q) == 2 == W["counts"]["flowing_links"] and q.view(np.int64)[0] == q.view(np.int64)[1] and q[0] > 0
    assert W["sums"]["Q_in"] == W["sums"]["Q_out"] == q[0] + q[1]


def test_the_stop_rules():
    M = du.random_discs(127, 121, N, 12700)
    net = nu.restate(M, N, -1)
    full = su.restate(M, N, T, 4, B, -1, 0, N=net)
    assert full["counts"]["status"] == 0 and full["counts"]["iterations"] > 33
    assert full["sums"]["rz"] <= 1e-16 * full["sums"]["rz0"]
    before = None
    for k in (1, 7, 33):
        W = su.restate(M, N, T, 4, B, -1, 0, max_iter=k, N=net)
        assert W["counts"]["status"] == 1 and W["counts"]["iterations"] == k
        assert before is None or W["sums"]["rz"] != before
        before = W["sums"]["rz"]
    # max_iter beyond what is needed changes nothing; 0 is the number of free regions
    assert su.same(su.restate(M, N, T, 4, B, -1, 0, max_iter=10 ** 6, N=net), full) is None
    assert full["limit"] == min(full["counts"]["free_regions"], su.AUTO_CAP)
    # status 2 needs dq <= 0 or not finite; with every g > 0 the matrix of the free regions is symmetric, diagonally dominant with a
    # positive diagonal, and d != 0 while rz != 0: it is unreachable here, and no case above meets it


def test_the_dot_is_the_tree_of_rule_4():
    rng = np.random.default_rng(4)
    for n in (1, 255, 256, 257, 65536, 65537, 70000):
        u, v = rng.standard_normal(n), rng.standard_normal(n)
        t = list(u * v)
        while True:
            t += [0.0] * (-len(t) % 256)
            nxt = []
            for blk in range(0, len(t), 256):
                w = t[blk:blk + 256]
                s = 128
                while s >= 1:
                    for i in range(s):
                        w[i] = w[i] + w[i + s]
                    s //= 2
                nxt.append(w[0])
            t = nxt
            if len(t) == 1:
                break
        assert np.float64(su.dot(u, v)).view(np.int64) == np.float64(t[0]).view(np.int64), n
    assert su.dot(np.zeros(0), np.zeros(0)) == 0.0


def _args(tmp_path, lx, ly, W, **kw):
    return dict(dict(directory=str(tmp_path), nFile=0, lx=lx, ly=ly, n=N, merge=-1, level=0, frm=T, band=4, to=B, links=W["table"],
                     solved=W["links"], region_body=W["region_body"], regions=W["regions"], counts=W["counts"], sums=W["sums"], t=0.0), **kw)


def test_write_netsolve_files_character_for_character(pkg, tmp_path):
    lx, ly = 40, 45
    for k, (merge, level) in enumerate(((-1, 0), (2, 1), (0, 1))):
        M = du.random_discs(lx, ly, N, k) if k < 2 else np.full((lx, ly), -1, np.int32)
        W = su.restate(M, N, T, 4, B, merge, level)
        t = 0.125 + 1e-3 * k
        pkg.write_netsolve_files(**_args(tmp_path, lx, ly, W, merge=merge, level=level, nFile=k, t=t))
        want = su.files_bytes(lx, ly, N, merge, level, T, 4, B, W, t, nfile=k)
        data = (tmp_path / "netsolve.data").read_bytes()
        assert data.startswith(su.DATA_HEADER.encode()) and data.endswith(want.pop("netsolve.data"))
        assert data.count(b"\n") == 2 + k
        for fname, text in want.items():
            assert (tmp_path / fname).read_bytes() == text, fname
    assert len(W["links"]) == 0 and len(W["regions"]) == 1          # the last: tables of no link


def test_write_netsolve_files_refusals(pkg, tmp_path):
    lx, ly = 40, 45
    M = du.random_discs(lx, ly, N, 1)
    W = su.restate(M, N, T, 4, B, -1, 0)
    assert len(W["links"]) >= 3 and len(W["regions"]) >= 3

    def text(**kw):
        with pytest.raises(pkg.LbmDemError) as e:
            pkg.write_netsolve_files(**dict(_args(tmp_path, lx, ly, W), **kw))
        assert e.value.code == -1
        return pkg.load_library().lbmdem_last_error().decode()
    assert "cannot open" in text(directory=str(tmp_path / "missing"))
    for kw in (dict(merge=-2), dict(level=2), dict(level=-1), dict(n=0), dict(frm=0), dict(frm=16), dict(to=0), dict(to=16), dict(band=0)):
        assert text(**kw) == "bad lbmdem_write_netsolve_files arguments"
    assert text(lx=1) == "lbmdem_write_netsolve_files: the lattice is 1 x %d" % ly
    assert text(solved=W["links"][:-1]) == "lbmdem_write_netsolve_files: there are %d links in the network and %d in the solution" % (
        len(W["links"]), len(W["links"]) - 1)
    assert text(links=W["table"][:-1]) == "lbmdem_write_netsolve_files: there are %d links in the network and %d in the solution" % (
        len(W["links"]) - 1, len(W["links"]))
    assert text(regions=W["regions"][:-1]) == "lbmdem_write_netsolve_files: there are %d body numbers and %d regions" % (
        len(W["regions"]), len(W["regions"]) - 1)
    assert text(region_body=W["region_body"][:-1]) == "lbmdem_write_netsolve_files: there are %d body numbers and %d regions" % (
        len(W["regions"]) - 1, len(W["regions"]))
    bad = W["table"].copy()
    bad[[1, 2]] = bad[[2, 1]]
    assert "the pairs ascend" in text(links=bad)
    bad = W["table"].copy()
    bad["hi"][0] = bad["lo"][0]
    assert "the pairs ascend, 0 <= lo < hi" in text(links=bad)
    bad = W["region_body"].copy()
    bad[2] = bad[1]
    assert "the bodies ascend" in text(region_body=bad)
    for flags in (-1, 8):
        bad = W["regions"].copy()
        bad["flags"][1] = flags
        assert text(regions=bad) == "lbmdem_write_netsolve_files: region 1 has the flags %d: 0 .. 7" % flags
    assert os.listdir(tmp_path) == []          # refused before anything is written
    for kw in (dict(counts=[0] * 9), dict(sums=[0.0] * 3)):
        with pytest.raises(pkg.LbmDemError):
            pkg.write_netsolve_files(**_args(tmp_path, lx, ly, W, **kw))
    # the float library has the formatter too
    if os.path.exists(pkg.SP_LIB_PATH):
        pkg.write_netsolve_files(**_args(tmp_path, lx, ly, W, precision="f32"))
        want = su.files_bytes(lx, ly, N, -1, 0, T, 4, B, W, 0.0)
        for fname in ("netsolve_regions000000.dat", "netsolve_links000000.dat"):
            assert (tmp_path / fname).read_bytes() == want[fname], fname


def test_symbols_and_methods_are_there(pkg):
    names = ("lbmdem_netsolve_compute lbmdem_download_netsolve_regions lbmdem_download_netsolve_links lbmdem_netsolve_rounds "
             "lbmdem_write_netsolve lbmdem_set_netsolve_output lbmdem_write_netsolve_files").split()
    for lib in (pkg.LIB_PATH, pkg.SP_LIB_PATH):
        if not os.path.exists(lib):
            continue
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
        assert not [s for s in names if s not in exported], lib
    for method in ("netsolve netsolve_regions netsolve_links netsolve_rounds netsolve_permeability write_netsolve "
                   "set_netsolve_output").split():
        assert callable(getattr(pkg.LbmDem, method)), method
    assert callable(pkg.write_netsolve_files) and pkg.NETSOLVE_COUNTERS == su.NETSOLVE_COUNTERS and len(pkg.NETSOLVE_COUNTERS) == 10
    assert pkg.NETSOLVE_SUMS == su.NETSOLVE_SUMS
    assert pkg.NETSOLVE_REGION_DTYPE == su.NETSOLVE_REGION_DTYPE and pkg.NETSOLVE_LINK_DTYPE == su.NETSOLVE_LINK_DTYPE
    assert pkg.NETSOLVE_REGION_DTYPE.itemsize == 24 and pkg.NETSOLVE_LINK_DTYPE.itemsize == 16
