"""CPU: the restatement of the cluster analysis (tests/cluster_util.py) against independent algorithms on random graphs, the
association of the threshold's sum, and lbmdem_write_clusters_files (include/lbmdem_hip.h), the host-only formatter, line for
line. No device is touched."""
import ctypes
import os
from collections import deque

import numpy as np
import pytest

import cluster_util as cl
import contacts_util as cu


def random_records(rng, n, npairs, nwalls):
    """pair records i < j without repeats, sorted as the export sorts them, then wall records; forces of a wide range"""
    pairs = set()
    while len(pairs) < min(npairs, n * (n - 1) // 2):
        i, j = sorted(rng.integers(0, n, 2).tolist())
        if i != j:
            pairs.add((i, j))
    walls = sorted({(int(rng.integers(0, n)), -int(rng.integers(1, 5))) for _ in range(nwalls)}, key=lambda w: (w[0], -w[1]))
    rec = np.zeros(len(pairs) + len(walls), cu.CONTACT_DTYPE)
    for k, (i, j) in enumerate(sorted(pairs) + walls):
        rec[k]["i"], rec[k]["j"] = i, j
    rec["fn"] = np.where(rng.random(len(rec)) < 0.15, 0.0, rng.lognormal(0.0, 1.5, len(rec)))
    return rec


def labels_bfs(n, pairs):
    adj = [[] for _ in range(n)]
    for i, j in pairs:
        adj[i].append(j)
        adj[j].append(i)
    label = [-1] * n
    for s in range(n):          # ascending: the first grain that reaches a component is its smallest
        if label[s] >= 0:
            continue
        label[s] = s
        q = deque([s])
        while q:
            a = q.popleft()
            for b in adj[a]:
                if label[b] < 0:
                    label[b] = s
                    q.append(b)
    return np.array(label, np.int32)


def core_one_by_one(n, pairs, wall_count, zmin, rng):
    """the peel with a worklist, one grain at a time, in a random order"""
    adj = [[] for _ in range(n)]
    for i, j in pairs:
        adj[i].append(j)
        adj[j].append(i)
    rem = [int(wall_count[i]) + len(adj[i]) for i in range(n)]
    alive = [True] * n
    work = [i for i in range(n) if rem[i] < zmin]
    while work:
        a = work.pop(int(rng.integers(0, len(work))))
        if not alive[a]:
            continue
        alive[a] = False
        for b in adj[a]:
            if alive[b]:
                rem[b] -= 1
                if rem[b] < zmin:
                    work.append(b)
    return np.array(alive, np.int32)


def test_restatement_against_bfs_and_another_peel_order():
    rng = np.random.default_rng(20)
    for case in range(300):
        n = int(rng.integers(1, 40))
        rec = random_records(rng, n, int(rng.integers(0, 2 * n + 1)), int(rng.integers(0, n + 1)))
        fmin, relative, zmin = float(rng.choice([0.0, 0.5, 1.0, 3.0])), bool(rng.integers(0, 2)), int(rng.integers(0, 5))
        x1, x2 = rng.random(n), rng.random(n)
        R = cl.restate(rec, n, x1, x2, fmin, relative, zmin)
        sel = rec[R["sel"]]
        pairs = [(int(c["i"]), int(c["j"])) for c in sel if c["j"] >= 0]
        wall_count = np.bincount(sel["i"][sel["j"] < 0], minlength=n)
        assert np.array_equal(R["label"], labels_bfs(n, pairs)), case
        assert np.array_equal(R["core"], core_one_by_one(n, pairs, wall_count, zmin, rng)), case
        # what the definitions say directly
        assert R["counts"]["selected_pairs"] == len(pairs) and R["counts"]["selected_walls"] == int(wall_count.sum())
        assert int(R["degree"].sum()) == 2 * len(pairs) + int(wall_count.sum())
        assert R["table"]["contacts"].sum() == len(pairs) and (R["table"]["size"] >= 2).all()
        assert (np.diff(R["table"]["label"]) > 0).all()
        core = R["core"].astype(bool)
        if zmin == 0:
            assert core.all()
        for i in np.nonzero(core)[0]:   # every survivor keeps zmin contacts among survivors and walls
            assert wall_count[i] + sum(1 for a, b in pairs if (a == i and core[b]) or (b == i and core[a])) >= zmin


def test_sum_chain_is_not_numpy_sum():
    # one large value in front and 1024 values that each vanish against it: the first block's chain loses every one of them,
    # a pairwise sum does not
    fn = np.concatenate([[2.0 ** 53], np.ones(1023), np.ones(1)])
    S, m = cl.s_chain(fn)
    assert m == 1025
    part0 = 0.0
    for v in fn[:1024]:
        part0 += float(v)
    part1 = 0.0
    part1 += float(fn[1024])
    spelled = 0.0
    spelled += part0
    spelled += part1
    assert S == spelled == 2.0 ** 53 and part0 == 2.0 ** 53   # (2^53 + 1 rounds back to 2^53, every time)
    assert float(np.sum(fn)) != S and float(np.sum(fn)) > 2.0 ** 53
    # records that are not positive are skipped, a NaN too
    S2, m2 = cl.s_chain(np.array([1.0, 0.0, np.nan, -3.0, 2.5]))
    assert (S2, m2) == (3.5, 2)
    rec = np.zeros(3, cu.CONTACT_DTYPE)
    rec["j"] = [1, 2, cu.WALL_B]
    rec["fn"] = [0.0, 0.0, 9.0]    # the wall's force is no part of the mean
    assert cl.threshold(rec, 1.0, True) == float("inf") and cl.threshold(rec, 0.0, True) == 0.0 and cl.threshold(rec, 2.0, False) == 2.0


def _grains():
    r = np.array([0.5e-3, 0.75e-3, 0.6e-3, 0.55e-3, 0.4e-3])
    x1 = np.array([1.0e-3, 2.2e-3, 3.5e-3, 4.6e-3, 6.0e-3])
    x2 = np.array([0.5e-3, 0.7e-3, 0.6e-3, 0.55e-3, 2.0e-3])
    fm = np.array([0.0, 0.25, 1.0, 0.5, 0.0])
    return r, x1, x2, fm


def _records():
    rec = np.zeros(6, cu.CONTACT_DTYPE)
    rec[0] = (0, 1, -1.5e-6, -0.986, -0.164, 2.4, -0.3)
    rec[1] = (1, 2, -1e-7, -1.0, 0.0, 0.0, 0.0)                 # touching, fn clamped to 0: below any positive threshold
    rec[2] = (2, 3, -2e-6, -1.0, 0.0, 3.2, 0.1)
    rec[3] = (0, cu.WALL_B, -2e-6, 0.0, 1.0, 6.0, 1.25e-300)
    rec[4] = (0, cu.WALL_L, -2e-6, 1.0, 0.0, 5.0, 0.0)
    rec[5] = (3, cu.WALL_R, -3e-6, -1.0, 0.0, -9.0, 4.194e+250)  # fn <= 0 at the right wall: never at or above a positive threshold
    return rec


@pytest.mark.parametrize("fmin,relative,zmin", [(0.5, True, 2), (0.0, False, 1), (2.5, False, 0)])
def test_files_are_exactly_the_expected_text(pkg, tmp_path, fmin, relative, zmin):
    r, x1, x2, fm = _grains()
    rec = _records()
    R = cl.restate(rec, len(r), x1, x2, fmin, relative, zmin)
    want = cl.files_text(r, x1, x2, fm, rec, R, fmin, relative, zmin, 0.125, 64, 48)
    for nfile in (7, 8):   # the second call appends its line to clusters.data, without another header
        pkg.write_clusters_files(str(tmp_path), nfile, r, x1, x2, fm, rec, R["label"], R["degree"], R["core"], R["walls"],
                                 R["table"], fmin, relative, zmin, R["thr"], R["counts"], 0.125, 64, 48)
    assert (tmp_path / "clusters000007.dat").read_text() == want[0]
    assert (tmp_path / "cluster_table000007.dat").read_text() == want[1]
    assert (tmp_path / "DEM000007_clusters.ps").read_text() == want[2]
    assert (tmp_path / "clusters.data").read_text() == cl.DATA_HEADER + want[3] + want[3]
    assert sorted(os.listdir(tmp_path)) == sorted(["clusters000007.dat", "cluster_table000007.dat", "DEM000007_clusters.ps",
                                                   "clusters000008.dat", "cluster_table000008.dat", "DEM000008_clusters.ps",
                                                   "clusters.data"])
    # format strings, line for line
    lines = want[0].splitlines()
    assert lines[0] == "# fmin %e relative %d zmin %d threshold %e" % (fmin, relative, zmin, R["thr"])
    assert lines[1] == "# i label degree core walls" and len(lines) == 2 + len(r)
    assert want[2].count("stroke") == int((R["sel"] & (rec["j"] >= 0)).sum()) == want[2].count("setrgbcolor")
    if (fmin, relative) == (0.5, True):   # half the mean of 2.4 and 3.2: both chains stay, in the colours of labels 0 and 2
        assert R["thr"] == 0.5 * ((0.0 + (0.0 + 2.4 + 3.2)) / 2.0) and R["label"].tolist() == [0, 0, 2, 2, 4]
        assert cl.PALETTE[0] in want[2] and cl.PALETTE[2] in want[2] and cl.PALETTE[1] not in want[2]
        assert want[1] == "0 2 1 5 %d %e %e %e %e\n2 2 1 0 %d %e %e %e %e\n" % (
            R["table"]["core"][0], x1[0], x1[1], x2[0], x2[1], R["table"]["core"][1], x1[2], x1[3], x2[3], x2[2])


def test_missing_directory_and_bad_records_are_refused(pkg, tmp_path):
    r, x1, x2, fm = _grains()
    rec = _records()
    R = cl.restate(rec, len(r), x1, x2, 1.0, True, 2)

    def write(d, records=rec, label=R["label"]):
        pkg.write_clusters_files(str(d), 0, r, x1, x2, fm, records, label, R["degree"], R["core"], R["walls"], R["table"], 1.0, True, 2,
                                 R["thr"], R["counts"], 0.0, 64, 48)
    with pytest.raises(pkg.LbmDemError, match="cannot open"):
        write(tmp_path / "not" / "there")
    for field, k, v in (("j", 0, 5), ("i", 2, -1), ("i", 3, 5), ("j", 4, -5)):
        bad = rec.copy()
        bad[field][k] = v
        with pytest.raises(pkg.LbmDemError, match=r"record %d names a grain outside \[0, 5\) or an unknown wall" % k) as e:
            write(tmp_path, records=bad)
        assert e.value.code == -1
    bad_label = R["label"].copy()
    bad_label[3] = 5
    with pytest.raises(pkg.LbmDemError, match=r"the label of grain 3 lies outside \[0, 5\)"):
        write(tmp_path, label=bad_label)
    assert os.listdir(tmp_path) == []      # refused before anything is written
    write(tmp_path)
    assert len(os.listdir(tmp_path)) == 4


def test_struct_and_both_libraries(pkg, tmp_path):
    assert pkg.CLUSTER_DTYPE == cl.CLUSTER_DTYPE and pkg.CLUSTER_DTYPE.itemsize == 56
    assert pkg.CLUSTER_COUNTERS == cl.COUNTERS and len(cl.COUNTERS) == 10
    if not os.path.exists(pkg.SP_LIB_PATH):
        pytest.skip("the single-precision library has not been built")
    r, x1, x2, fm = _grains()
    rec = _records()
    R = cl.restate(rec, len(r), x1, x2, 1.0, True, 2)
    pkg.write_clusters_files(str(tmp_path), 1, r, x1, x2, fm, rec, R["label"], R["degree"], R["core"], R["walls"], R["table"], 1.0,
                             True, 2, R["thr"], R["counts"], 0.5, 64, 48, precision="f32")
    want = cl.files_text(r, x1, x2, fm, rec, R, 1.0, True, 2, 0.5, 64, 48)
    assert (tmp_path / "clusters000001.dat").read_text() == want[0]
    assert (tmp_path / "clusters.data").read_text() == cl.DATA_HEADER + want[3]
