"""GPU: odd and ragged lattice shapes.

The fused fluid kernel marches over the rows in segments (8 rows on every small lattice, unrolled by two) and over the columns
in windows of 60 producing lanes; the frame and checkpoint kernels work in tiles and 16-byte chunks. The S_* cases
(tests/golden/make_golden.py: lx % 8 = 1 ... 7, ly % 60 in {0, 1, 2, 3, 17, 59}, no ly a multiple of the row pitch's 16 / 32,
grains clipped by all four walls where lx >= 60, odd grain counts) were dumped from the unmodified reference; here the change mask, the VTK
writers, the checkpoints and the strip decomposition run on them. Then the segment lengths no other test runs (12, 18 and
uniform 32 rows with a short last segment, the tapered order on an odd row count) and a fuzz sweep on ragged lattices, both
against the CPU oracle (which tests/test_oracle_golden.py pins to the reference on the S_* shapes). All comparisons are exact."""
import ctypes
import os

import numpy as np
import pytest

import fuzz_util
import golden_util as gu
import samples

pytestmark = pytest.mark.gpu

SHAPE_CASES = sorted(k for k, v in gu.CASES.items() if v["kind"] == "shape")
COLS9 = list(range(9))


def end_state(sim):
    """the last dump of run_shape_case, from a handle that is already there"""
    f, obst, fhf, kin = sim.f, sim.obst, sim.fhf, sim.kinematics
    return {"sha_f_end": gu.sha(f), "sha_obst_end": gu.sha(obst.astype(np.int32)), "sha_fhf_end": gu.sha(fhf),
            "sha_kin_end": gu.sha(kin), "density_end": np.float64(sim.final_density()),
            "f_end": f, "obst_end": obst, "fhf_end": fhf, "grains_end": kin}


def start(pkg, name):
    """-> (adapter with the case's agitated grains uploaded, sub-steps of the whole run)"""
    a = gu.GpuAdapter(pkg, name)
    c = gu.CASES[name]
    a.set_kinematics(gu.mg.shape_initial_kinematics(c))
    return a, c["dumps"][-1] * a.sim.cfg.npDEM + 5


# ---- 1. the change mask ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SHAPE_CASES)
def test_change_mask_on_ragged_shapes(pkg, name):
    """the per-window change bits (one word per 32 rows, padded by four) on lattices of 13 ... 203 rows: verified at every use
    (mode 2), and both that handle and one that reads both maps everywhere on the reference's digests at every dump"""
    lx = gu.CASES[name]["lx"]
    for mode in (2, 0):
        a = gu.GpuAdapter(pkg, name)
        a.sim.set_change_mask(mode)
        res = gu.run_case(a, name)
        gu.compare(name, res, grain_cols=COLS9)
        used, hidden = a.sim.change_mask_stats()
        print(f"{name} mode {mode}: fused launches on the change bits {used}, hidden differences {hidden}")
        assert hidden == 0, (mode, hidden)
        if mode == 0:
            assert used == 0
        elif lx >= 60:
            assert used > 0
        a.sim.close()


# ---- 2. VTK frames ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["S_61x59", "S_127x121"])
def test_vtk_frames_on_ragged_shapes(pkg, tmp_path, name):
    """write_vtk and write_vtk_async (the transposing snapshot kernel) after the case's last dump: the same five files, and on
    61 x 59 the reference's own (tests/golden/vtk_S_61x59/)"""
    a = gu.GpuAdapter(pkg, name)
    gu.compare(name, gu.run_case(a, name), grain_cols=COLS9)
    ds, da = tmp_path / "sync", tmp_path / "async"
    ds.mkdir(); da.mkdir()
    nfile = gu.mg.VTK_NFILE
    a.sim.write_vtk(str(ds), nfile)
    a.sim.set_async_output(2)
    a.sim.write_vtk_async(str(da), nfile)
    a.sim.output_drain()
    names = sorted(p.name for p in ds.iterdir())
    assert len(names) == 5 and names == sorted(p.name for p in da.iterdir()), names
    for n in names:
        assert (ds / n).read_bytes() == (da / n).read_bytes(), n
    ref_dir = os.path.join(gu.HERE, "golden", "vtk_" + name)
    if name == "S_61x59":
        assert sorted(os.listdir(ref_dir)) == names
    if os.path.isdir(ref_dir):
        for n in names:
            got, want = (ds / n).read_bytes(), open(os.path.join(ref_dir, n), "rb").read()
            assert got == want, f"{n}: {len(got)} vs {len(want)} bytes, first diff at " \
                                f"{next((i for i, (u, v) in enumerate(zip(got, want)) if u != v), None)}"
    a.sim.close()


# ---- 3. checkpoints ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["S_61x59", "S_127x121"])
def test_checkpoints_on_ragged_shapes(pkg, tmp_path, name):
    """an odd grain count (the grains' sections start 8 or 4 bytes into a 16-byte chunk, wallflags and offsets end inside one)
    on a lattice whose row pitch is not ly: the background file is the synchronous one plus its trailer and verifies; the
    checkpoint taken after the third fluid period, loaded, ends the run on the reference's final dump"""
    from test_gpu_async_checkpoint import check_async_file
    a, total = start(pkg, name)
    g = gu.load(name)
    assert a.sim.n % 2 == 1 and a.sim.ly % 16 != 0
    a.sim.set_async_checkpoint(1)
    third = 3 * a.sim.cfg.npDEM
    a.steps(third)
    S, A = str(tmp_path / "sync.ckpt"), str(tmp_path / "async.ckpt")
    a.sim.checkpoint_save_async(A)
    a.sim.checkpoint_save(S)
    a.steps(total - third)             # at once: nothing stepped here may reach the file
    a.sim.output_drain()
    check_async_file(A, S, a.sim)
    assert pkg.LbmDem.checkpoint_verify(A) is True and pkg.LbmDem.checkpoint_verify(S) is False
    gu.compare(name, end_state(a.sim), grain_cols=COLS9)
    for path in (A, S):
        b = pkg.LbmDem.checkpoint_load(path)
        assert b.nbsteps == third and b.n == a.sim.n
        assert gu.sha(b.f) == str(g["sha_f_3"]) and gu.sha(b.obst.astype(np.int32)) == str(g["sha_obst_3"])
        assert gu.sha(b.kinematics) == str(g["sha_kin_3"]) and gu.sha(b.fhf) == str(g["sha_fhf_3"])
        b.renderScene(total - third)
        gu.compare(name, end_state(b), grain_cols=COLS9)
        b.close()
    a.sim.close()


# ---- 4. strips ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def single_203x122(pkg):
    """S_203x122 on one domain: its last dump and the number of sub-steps (computed once, read by both strip counts)"""
    a, total = start(pkg, "S_203x122")
    a.steps(total)
    out = dict(end_state(a.sim), total=total)
    a.sim.close()
    return out


@pytest.mark.parametrize("world", [2, 3])
def test_strips_of_an_odd_lattice_equal_one_domain(pkg, single_203x122, world):
    """203 x 122 in 2 strips (101 + 102 rows) and in 3 (67 + 68 + 68): the rows next to a cut are ranges of halo = 11 rows, an
    odd width -- one launch for both ranges of the middle strip (launch_march_two_ranges), a launch of its own next to a single
    cut -- and the interiors have odd row counts too. Replicated grains, loop-back messages; against one domain and against the
    reference's final dump, the serial total density (each strip continuing its predecessor's sum) included. (lbmdem_create accepts every one of these strips: none is narrower than its halos.)"""
    import torch
    from strip_backends import LoopbackComm, lockstep_render
    strips = pkg.strips_module()
    name = "S_203x122"
    c = gu.CASES[name]
    lx, ly = c["lx"], c["ly"]
    r, x1, x2 = gu.inputs_m(name)
    k0 = gu.mg.shape_initial_kinematics(c)
    single = single_203x122
    cfg = pkg.derive(lx, ly, r)
    halo = strips.halo_rows(float(r.max()), cfg.dx)
    parts = strips.partition(lx, world)
    assert halo % 2 == 1 and all(b - a > 2 * halo for a, b in parts)
    runners = []
    for rank, strip in enumerate(parts):
        be = strips.GpuStripBackend(pkg, torch, lx, ly, r, x1, x2, strip, halo, 0)
        be.sim.kinematics = k0
        runners.append(strips.StripRunner(be, LoopbackComm(), rank, world))
    lockstep_render(runners, single["total"])
    f = np.full((lx, ly, 9), np.nan)
    obst = np.full((lx, ly), -7, np.int32)
    for R in runners:
        s = R.b.sim
        s.sync()
        s.download_f_into(f)
        s._L.lbmdem_download_obst(s._h, obst.ctypes.data_as(ctypes.c_void_p))
        assert np.array_equal(s.kinematics, single["grains_end"])
        assert np.array_equal(s.fhf, single["fhf_end"])
    assert np.array_equal(f, single["f_end"])
    assert np.array_equal(obst, single["obst_end"])
    tot = 0.0
    for R in runners:       # every strip continues from its predecessor's sum
        tot = R.b.sim.final_density(tot)
    assert tot == single["density_end"]
    s = runners[0].b.sim
    gu.compare(name, {"sha_f_end": gu.sha(f), "sha_obst_end": gu.sha(obst), "f_end": f, "obst_end": obst, "fhf_end": s.fhf,
                      "grains_end": s.kinematics, "sha_kin_end": gu.sha(s.kinematics), "sha_fhf_end": gu.sha(s.fhf),
                      "density_end": np.float64(tot)}, grain_cols=COLS9)
    for R in runners:
        R.b.sim.close()


# ---- 5. segment lengths nobody runs -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("lx,ly,levels,seg,last", [
    (1003, 3000, 0, 12, 7),      # run-time segments of 12 rows, the last one 7: its fourth pair is half silenced
    (1531, 3000, 0, 18, 1),      # 18 rows, the last segment a single row
    (1031, 7700, 0, 32, 7),      # uniform 32-row segments on >= 1024 rows: the tapered plan declines (bands of 192 rows = its tail)
    (2047, 3901, 4, 64, None),   # the tapered order on an odd row count: the last band is one row short
])
def test_segment_lengths_with_a_short_last_segment(pkg, po, lx, ly, levels, seg, last):
    """march_segment_rows gives rows / ceil(4096 / windows), even, within 8 ... 32; the suite's other lattices make that 8, 16 at
    2048^2, or hand over to the tapered order. Two fluid steps and the sub-steps between them, every array against the oracle."""
    r, x, y = samples.row_packing(lx, ly, 4000, seed=lx + ly)
    r, x1, x2 = samples.to_metres(r, x, y)
    sim = pkg.LbmDem(lx, ly, r, x1, x2)
    wo = sim.fused_work_order()
    print(f"{lx}x{ly}: {len(r)} grains, work order {wo}")
    assert wo["levels"] == levels and wo["segment_rows"][0] == seg, wo
    if levels == 0:
        assert wo["segment_rows"] == [seg] and lx % seg == last and wo["items"] == -(-ly // 60) * -(-lx // seg), wo
    else:
        assert wo["segment_rows"] == [64, 32, 16, 8] and 8 * wo["band_rows"] - lx == 1 and lx % 2 == 1, wo
    ora = po.Oracle(lx, ly, r, x1, x2)
    k = sim.cfg.npDEM + 1   # fluid steps at nbsteps 0 and npDEM
    sim.renderScene(k); ora.steps(k)
    assert ora.act_anomalies() == 0
    assert np.array_equal(sim.obst, ora.get_obst())
    assert np.array_equal(sim.f, ora.get_f())
    assert np.array_equal(sim.fhf, ora.get_fhf())
    assert np.array_equal(sim.kinematics, ora.get_grains()[:, :9])
    sim.close()


# ---- 6. ragged fuzz ---------------------------------------------------------------------------------------------------------

def ragged_shapes(count, seed=2027):
    """lx in [65, 260] and no multiple of 8, ly in [61, 260]"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        lx, ly = int(rng.integers(65, 261)), int(rng.integers(61, 261))
        if lx % 8 != 0:
            out.append((lx, ly))
    return out


@pytest.mark.parametrize("seed,shape", list(zip(range(6001, 6009), ragged_shapes(8))))
def test_random_packing_on_a_ragged_lattice_is_bit_equal_to_the_oracle(pkg, po, seed, shape):
    desc, ok, tab, gat, _ = fuzz_util.run_case(pkg, po, seed, shape=shape)
    assert ok is not None, desc
    assert ok, desc
    assert tab > 0, desc        # the link-sum table served grains (not everything fell to the gather queue)
