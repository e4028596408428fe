"""GPU: the DEM and coupling paths on two-dimensional packings (tests/packing_util.py: jittered triangular lattices).

Every other synthetic scene of the suite is laid in rows that never touch each other (samples.row_packing): a grain there
carries at most two non-zero contact forces -- a sum of two terms cannot depend on the order of the additions --, every
contact normal is horizontal, and a reduced disc meets at most two others. Here more than half of the grains carry three or
more contacts, two thirds of the normals are 60 degrees from horizontal and at reductionR 1.08 a reduced disc meets six
others: the order in which k_dem_chain's tiles, the per-sub-step kernels, the distributed-grain kernels and the merge across
a strip cut add a grain's forces, the `yn` terms of the contact laws and the hand-over of map nodes among several partners
decide bits. Each test repeats, on such a scene, a comparison another file makes on rows; the scene's census is asserted
first (numpy, inputs only), so a change of parameters cannot quietly turn the inputs back into rows. The CPU oracle these
tests compare with is pinned to the unmodified reference on the same packings (tests/test_packing_host.py, and the golden
case P_tri_127x121). All comparisons are exact."""
import ctypes

import numpy as np
import pytest

import contacts_util as cu
import fuzz_util
import packing_util as pu
from strip_backends import LoopbackComm, lockstep_render, lockstep_render_dist
from test_gpu_contacts import restated, table_substep
from test_gpu_dem_chain import kick
from test_gpu_obst_update import check, trio
from test_gpu_shapes import ragged_shapes

pytestmark = pytest.mark.gpu


def scene(lx, ly, rmean, shuffle=False, **kw):
    """-> (r, x1, x2) in metres, after the census of the scene"""
    r, x, y = pu.tri_packing(lx, ly, rmean, shuffle=shuffle, **kw)
    c = pu.check_scene(lx, ly, r, x, y, (lx, ly, rmean))
    assert c["touching_pairs"] > c["grains"], c
    return pu.samples.to_metres(r, x, y)


# ---- 1. the coupled step against the oracle -----------------------------------------------------------------------------

@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("lx,ly,rmean", [(256, 200, 0.7), (127, 121, 0.5)])
def test_coupled_parity_with_the_oracle(pkg, po, lx, ly, rmean, shuffle):
    """nine fluid periods and more (past the list rebuild at sub-step 100) from kicked grains: fhf and the nine kinematic
    columns after every period, f and the map at the end"""
    r, x1, x2 = scene(lx, ly, rmean, shuffle)
    sim = pkg.LbmDem(lx, ly, r, x1, x2)
    ora = po.Oracle(lx, ly, r, x1, x2)
    ora.set_kinematics(kick([sim], len(r), 17))
    n = sim.cfg.npDEM
    periods = max(9, 100 // n + 2)
    tab = 0
    for p in range(periods):
        sim.renderScene(n); ora.steps(n)
        assert np.array_equal(sim.fhf, ora.get_fhf()), (shuffle, sim.nbsteps)
        assert np.array_equal(sim.kinematics, ora.get_grains()[:, :9]), (shuffle, sim.nbsteps)
        tab += sim.force_stats()[0]
    assert sim.nbsteps > 100 + n
    assert np.array_equal(sim.f, ora.get_f())
    assert np.array_equal(sim.obst, ora.get_obst())
    assert ora.act_anomalies() == 0
    assert tab > 0, "the link-sum table served no grain: everything fell to the gather queue"
    sim.close()


# ---- 2. the multi-sub-step kernel, its tiles and the numbering ----------------------------------------------------------

def chain_scene():
    """256 x 200, 0.35 mm grains numbered at random: 1136 grains, about 18 tiles with halos in every direction"""
    lx, ly = 256, 200
    r, x1, x2 = scene(lx, ly, 0.35, shuffle=True)
    assert len(r) == 1136
    return lx, ly, r, x1, x2


@pytest.mark.parametrize("tiles", [1, 0])
def test_chain_equals_one_launch_per_substep(pkg, tiles):
    lx, ly, r, x1, x2 = chain_scene()
    a = pkg.LbmDem(lx, ly, r, x1, x2)
    a.set_dem_tiles(tiles)
    b = pkg.LbmDem(lx, ly, r, x1, x2)
    b.set_dem_chain(0)
    kick([a, b], len(r), 17)
    runs = (37, 1, 12, 200, 95)     # runs of every length, across fluid steps and list rebuilds
    for n in runs:
        a.renderScene(n); b.renderScene(n)
        assert a.nbsteps == b.nbsteps
        assert np.array_equal(a.kinematics, b.kinematics), (tiles, a.nbsteps)
        assert np.array_equal(a.grain_pressure, b.grain_pressure), (tiles, a.nbsteps)
        assert np.array_equal(a.fhf, b.fhf), (tiles, a.nbsteps)
    assert np.array_equal(a.f, b.f)
    assert np.array_equal(a.obst, b.obst)
    la, sa, slots, resident = a.dem_chain_stats()
    # the chain did run: all tiles resident, a launch in every fluid period at least (every fluid step ends one; on the rows of
    # tests/test_gpu_dem_chain.py, npDEM 12, that reads 28: it asks for 30 there), nearly all sub-steps inside launches
    assert resident == slots and la >= sum(runs) // a.cfg.npDEM and sa >= 300, \
        f"the multi-sub-step kernel declined on this scene: {(la, sa, slots, resident)}"
    assert b.dem_chain_stats()[:2] == (0, 0)
    a.close(); b.close()


def test_chain_dem_only_long_runs_match_oracle(pkg, po):
    """run_dem (the reference without _FLUIDE_): runs of 100 sub-steps between list rebuilds"""
    lx, ly, r, x1, x2 = chain_scene()
    sim = pkg.LbmDem(lx, ly, r, x1, x2)
    ora = po.Oracle(lx, ly, r, x1, x2)
    ora.set_kinematics(kick([sim], len(r), 3))
    for n in (250, 333):
        sim.run_dem(n); ora.steps_dry(n)
        assert np.array_equal(sim.kinematics, ora.get_grains()[:, :9]), sim.nbsteps
    assert sim.dem_chain_stats()[1] >= 570, \
        f"the multi-sub-step kernel declined on this scene: {sim.dem_chain_stats()}"      # all but a handful of the 583
    sim.close()


# ---- 3. the contact export, record by record ----------------------------------------------------------------------------

@pytest.mark.parametrize("nbsteps", [0, 1])
def test_contact_export_record_by_record(pkg, nbsteps):
    """a table sub-step from random velocities and accelerations (nbsteps 0: the film law): more contacts than grains -- no
    row packing has that --, Coulomb-clamped ones, force-free ones, grains pressed into the floor"""
    lx, ly, r, x1, x2, k = pu.contact_scene()
    pu.check_scene_m(lx, ly, r, x1, x2, "contact scene")
    n = len(r)
    with pkg.LbmDem(lx, ly, r, x1, x2) as sim:
        pre, film = table_substep(sim, k, nbsteps)
        assert film == (nbsteps == 0)
        rec, stats = sim.download_contacts(), sim.contact_stats()
        want, counts, _ = restated(sim, pre, film)
        assert counts["touching_pairs"] >= n and counts["coulomb_clamped"] > 0 and counts["fn_zero"] > 0, counts
        assert counts["wall_contacts"] >= 6, counts
        assert cu.same_records(rec, want), (len(rec), len(want))
        assert stats == counts, (stats, counts)
        # per grain: three and more records with a steep normal among them
        pairs = rec[rec["j"] >= 0]
        per = np.bincount(np.concatenate([pairs["i"], pairs["j"]]), minlength=n)
        assert (per >= 3).mean() >= pu.MIN_FRAC_3_PARTNERS and (np.abs(pairs["ny"]) > np.abs(pairs["nx"])).mean() >= pu.MIN_FRAC_STEEP
        assert np.array_equal(sim.download_contacts(), rec)   # asking again changes nothing


# ---- 4. the map updated in place, with many overlapping partners --------------------------------------------------------

@pytest.mark.parametrize("reduction", [1.0, 1.08])
def test_overlapping_reduced_discs_of_many_partners_that_move(pkg, po, reduction):
    """update, clear + repaint and the oracle: at 1.08 a reduced disc meets its six lattice neighbours' (rows: two), so the
    compare-and-swap hand-over chooses among several partners whose new discs cover a node"""
    lx, ly = 200, 150
    r, x1, x2 = scene(lx, ly, 0.6)
    many = (pu.reduced_disc_partners(r, x1, x2, reduction) >= 3).mean()
    assert reduction < 1.08 or many >= 0.30, many
    a, b, ora = trio(pkg, po, lx, ly, r, x1, x2, reduction=reduction, vel=(0.4, 0.4, 30.0), seed=2)
    n = a.cfg.npDEM
    for k in range(10):
        a.renderScene(2 * n + 1); b.renderScene(2 * n + 1); ora.steps(2 * n + 1)
        check(a, b, ora, f"reductionR {reduction}, step {a.nbsteps}")
    assert np.array_equal(a.f, ora.get_f())
    assert a.obst_stats()[0] > 10, a.obst_stats()
    a.close(); b.close()


# ---- 5. strips ----------------------------------------------------------------------------------------------------------

def cut_conditions(r, x1, x2, parts, dx):
    """across each cut at least five touching pairs with centres on opposite sides, and at least three grains with two or
    more touching partners beyond the cut as well as two or more on their own side (the initial state, numpy)"""
    for a, _ in parts[1:]:
        across, both = pu.cut_census(r, x1, x2, a * dx)
        assert across >= 5 and both >= 3, (a, across, both)


def single_domain(pkg, lx, ly, r, x1, x2, k, nsteps):
    s = pkg.LbmDem(lx, ly, r, x1, x2)
    s.kinematics = k
    s.renderScene(nsteps)
    out = dict(f=s.f, obst=s.obst, fhf=s.fhf, kin=s.kinematics, density=s.final_density())
    s.close()
    return out


def gathered(runners, lx, ly):
    f = np.full((lx, ly, 9), np.nan)
    obst = np.full((lx, ly), -7, np.int32)
    tot = 0.0
    for R in runners:       # the serial total density: every strip continues from its predecessor's sum
        s = R.b.sim
        s.sync()
        s.download_f_into(f)
        s._L.lbmdem_download_obst(s._h, obst.ctypes.data_as(ctypes.c_void_p))
        tot = s.final_density(tot)
    return f, obst, tot


@pytest.mark.parametrize("world", [2, 3])
def test_strips_with_replicated_grains_equal_one_domain(pkg, world):
    """203 x 122 (lbmdem_create accepts every strip at this size), loop-back messages. The lattice is laid 0.2 mm from the
    walls for two strips and 0.05 mm for three: with one margin for both, one of the cuts has fewer than three grains with two
    partners on either side."""
    import torch
    strips = pkg.strips_module()
    lx, ly = 203, 122
    r, x1, x2 = scene(lx, ly, 0.5, margin={2: 0.2, 3: 0.05}[world])
    cfg = pkg.derive(lx, ly, r)
    parts = strips.partition(lx, world)
    cut_conditions(r, x1, x2, parts, cfg.dx)
    halo = strips.halo_rows(float(r.max()), cfg.dx)
    assert all(b - a > 2 * halo for a, b in parts)
    k = pu.agitation(len(r), seed=2, scale=(0.03, 0.03, 20.0)); k[:, 0], k[:, 1] = x1, x2
    nsteps = 9 * cfg.npDEM + 3
    assert nsteps > 100
    runners = []
    for rank, strip in enumerate(parts):
        be = strips.GpuStripBackend(pkg, torch, lx, ly, r, x1, x2, strip, halo, 0)
        be.sim.kinematics = k
        runners.append(strips.StripRunner(be, LoopbackComm(), rank, world))
    lockstep_render(runners, nsteps)
    one = single_domain(pkg, lx, ly, r, x1, x2, k, nsteps)
    f, obst, tot = gathered(runners, lx, ly)
    assert np.array_equal(f, one["f"])
    assert np.array_equal(obst, one["obst"])
    for R in runners:
        assert np.array_equal(R.b.sim.kinematics, one["kin"])
        assert np.array_equal(R.b.sim.fhf, one["fhf"])
    assert tot == one["density"]
    for R in runners:
        R.b.sim.close()


@pytest.mark.parametrize("world", [2, 3])
def test_strips_with_distributed_grains_equal_one_domain(pkg, world):
    """687 x 122: the narrowest odd lattice whose thirds (229 rows) hold the margin of grains a rank integrates beyond its
    cuts (222 rows at npDEM 13) -- lbmdem_dist_enable refuses a strip narrower than that, 203 x 122 in particular -- and whose
    cuts, in 2 and in 3 strips, have the contacts asked for. Every rank overwrites the grains it does not integrate with NaN."""
    import torch
    strips = pkg.strips_module()
    lx, ly = 687, 122
    r, x1, x2 = scene(lx, ly, 0.5)
    cfg = pkg.derive(lx, ly, r)
    parts = strips.partition(lx, world)
    cut_conditions(r, x1, x2, parts, cfg.dx)
    margin = strips.default_margin(cfg.npDEM, float(r.max()), cfg.phys.distVerlet, cfg.dx)
    assert min(b - a for a, b in parts) >= margin
    k = pu.agitation(len(r), seed=5, scale=(0.05, 0.03, 20.0)); k[:, 0], k[:, 1] = x1, x2
    nsteps = 9 * cfg.npDEM + 5
    assert nsteps > 100
    runners = []
    for rank, strip in enumerate(parts):
        be = strips.GpuStripBackend(pkg, torch, lx, ly, r, x1, x2, strip, 2, 0, distributed=True, margin=margin, poison=True)
        be.sim.kinematics = k
        runners.append(strips.DistStripRunner(be, LoopbackComm(), rank, world))
    lockstep_render_dist(runners, nsteps)
    one = single_domain(pkg, lx, ly, r, x1, x2, k, nsteps)
    f, obst, tot = gathered(runners, lx, ly)
    assert np.array_equal(f, one["f"])
    assert np.array_equal(obst, one["obst"])
    xc = one["kin"][:, 0] / cfg.dx
    for R, (a, b) in zip(runners, parts):       # a rank answers for the grains it owns
        own = ((a == 0) | (xc >= a)) & ((b == lx) | (xc < b))
        assert own.sum() > 0
        assert np.array_equal(R.b.sim.kinematics[own], one["kin"][own])
        assert np.array_equal(R.b.sim.fhf[own], one["fhf"][own])
    assert tot == one["density"]
    for R in runners:
        R.b.sim.close()


# ---- 6. fuzz ------------------------------------------------------------------------------------------------------------

RAGGED = ragged_shapes(8)
# seeds whose laid packing passes packing_util.check_scene (run_case asserts it): chosen from the census alone
FUZZ = [(7001, None), (7003, None), (7006, None), (7008, None),
        (7101, RAGGED[0]), (7103, RAGGED[2]), (7104, RAGGED[3]), (7108, RAGGED[7])]


@pytest.mark.parametrize("seed,shape", FUZZ)
def test_random_triangular_packing_is_bit_equal_to_the_oracle(pkg, po, seed, shape):
    desc, ok, tab, gat, _ = fuzz_util.run_case(pkg, po, seed, shape=shape, packing="tri")
    assert ok is not None, desc
    assert ok, desc
    assert tab > 0, desc        # the link-sum table served grains (not everything fell to the gather queue)
