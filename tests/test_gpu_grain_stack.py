"""GPU: the contact export, the clusters, the packing structure and the Voronoi cells on ONE handle, with the coarse and the flow
fields between them, in any order (include/lbmdem_hip.h, "The contact network export" through "Voronoi cells"). The single stages'
tests hold every output to its restatement; here the chain is held to the model of tests/grain_stack_util.py (pinned by
tests/test_grain_stack_host.py): after every operation every reader of the four stateful stages either answers with the restatement
of the compute the model says it belongs to -- doubles on the bits, integers by array_equal -- or is refused with the stage's own
sentence. Downloading readers only, except in the one test of the device views.

The scene is grain_stack_util.scene(): shape_packing(65) of the single stages' files with one grain pressed into the left and one
into the right wall (tests/test_grain_stack_host.py shows that it meets every inequality the comparisons need), on a handle whose
lbmdem_move_walls gives both side walls another value (amp 2 um) or, where a test says so, the same value (amp 0)."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import grain_stack_util as gs

pytestmark = pytest.mark.gpu
o = gs.op
P0, P1 = gs.CLUSTER_PARAMS
S0, S1, SC = gs.STRUCTURE_PARAMS


class Stack:
    """a handle on the scene (and a twin, for the walks) with its harness"""

    def __init__(self, pkg, tmp_path, shaking=True, twin=False, tag=""):
        lx, ly, r, k = gs.scene()
        phys = gs.physics(pkg, lx, ly, r, shaking)
        self.sims = [pkg.LbmDem(lx, ly, r, k[:, 0], k[:, 1], physics=phys) for _ in range(2 if twin else 1)]
        self.h = gs.Harness(pkg, self.sims[0], r, k, shaking, tmp_path, twin=self.sims[1] if twin else None, tag=tag)

    def __enter__(self):
        return self.h

    def __exit__(self, *a):
        for s in self.sims:
            s.close()


def run_all(h, ops, check=True):
    for op_ in ops:
        h.run(op_)
        if check:
            h.check_all()


FIRST = gs.operations(True)
# two of the model's three prepared states: with all three the file took more than twice the slowest single stage's file (LABBOOK,
# "The grain analyses as one chain"); the third, only structure and contacts computed, stays with the model's completeness on the CPU
PAIR_STATES = ("everything", "nothing")


@pytest.mark.parametrize("first", range(len(FIRST)), ids=[gs.show(a).replace(" ", "") for a in FIRST])
def test_ordered_pairs(pkg, tmp_path, first):
    """A, then B, for every B, from each of two prepared states (everything computed, nothing computed): every reader after A and
    after B. The handle's lbmdem_move_walls gives the walls another value"""
    with Stack(pkg, tmp_path, tag="pairs from %s:" % gs.show(FIRST[first])) as h:
        for state in PAIR_STATES:
            for second in FIRST:
                run_all(h, (gs.RESET,) + gs.STATES[state], check=False)
                run_all(h, [FIRST[first], second])


def test_ordered_pairs_with_a_move_to_the_same_value(pkg, tmp_path):
    """the pairs (move, B) and (A, move) on a handle whose lbmdem_move_walls changes no wall's bits (amp = 0): nothing changes"""
    move, ops = o("move_walls_same"), gs.operations(False)
    with Stack(pkg, tmp_path, shaking=False, tag="pairs with a still move:") as h:
        for state in PAIR_STATES:
            for other in ops:
                for pair in ((move, other), (other, move)):
                    run_all(h, (gs.RESET,) + gs.STATES[state], check=False)
                    run_all(h, pair)


def test_the_four_stages_at_two_parametrisations_in_all_orders(pkg, tmp_path):
    """contacts, clusters, structure and Voronoi in all 24 orders, each stage at its two parametrisations one after the other, every
    reader after each compute: a reader answers with the parameters its own last compute was given, whatever ran since"""
    with Stack(pkg, tmp_path, tag="all orders:") as h:
        for order in itertools.permutations(gs.STAGES):
            h.run(gs.RESET)
            for stage in order:
                run_all(h, gs.TWO_EACH[stage])
            assert h.model.expect("contacts", "lbmdem_download_contacts").state == "answers"
            assert h.model.expect("clusters", "lbmdem_download_clusters").result["p"] == P1
            assert h.model.expect("structure", "lbmdem_download_structure_hist").result["rcut"] in (S1[0], gs.WRITE_VORONOI)


@pytest.mark.parametrize("seed", gs.SEEDS)
def test_seeded_walks(pkg, tmp_path, seed):
    """40 operations of the full list, every reader held to the model after each; a failure names the seed, the operation and the
    operations up to it. A twin handle makes the steps and no analysis: what a step reads ends up equal, and so do the contacts"""
    with Stack(pkg, tmp_path, shaking=seed != gs.STILL_SEED, twin=True, tag="walk of seed %d:" % seed) as h:
        run_all(h, [gs.RESET] + gs.walk(seed))
        h.undisturbed()
        for s in (h.sim, h.twin):
            s.set_diagnostics(True)
            s.dem_substep()
        assert gs.cu.same_records(h.sim.download_contacts(), h.twin.download_contacts())


# ---- the six questions ----

def test_q1_a_second_structure_compute_leaves_the_voronoi_cells(pkg, tmp_path):
    """Voronoi cells: "The cells are the Voronoi stage's own: a later lbmdem_structure_compute (another rcut or nbins, counts only,
    refused) leaves the readers answering with the cells of the list and the rcut they were made with". Packing structure: "a later
    compute replaces the result whole". The Voronoi readers go on giving the cells of the first rcut, the structure readers describe
    the second compute; `# rcut` of voronoi%.6i.dat is lbmdem_write_voronoi's own argument (the harness compares the file)"""
    with Stack(pkg, tmp_path, tag="q1:") as h:
        run_all(h, [gs.RESET, o("structure", p=S0), o("voronoi")])
        for second in (o("structure", p=S1), o("structure", p=SC), o("write_structure", p=gs.WRITE_STRUCTURE)):
            run_all(h, [second])
            assert h.model.expect("voronoi", "lbmdem_download_voronoi_faces").result["rcut"] == S0[0]
        with pytest.raises(pkg.LbmDemError, match="nbins must lie in 1 .. 4096"):          # refused for a parameter: nothing changes
            h.sim.structure(S1[0] * h.D, 0, 1.2)
        h.check_all()
        run_all(h, [o("structure", p=S1), o("voronoi"), o("structure", p=S0)])
        assert h.model.expect("voronoi", "lbmdem_download_voronoi_faces").result["rcut"] == S1[0]
        run_all(h, [o("write_voronoi", rcut=gs.WRITE_VORONOI)])


def test_q2_write_voronoi_leaves_its_own_structure_compute(pkg, tmp_path):
    """Voronoi cells: lbmdem_write_voronoi makes "lbmdem_structure_compute(rcut, 1, 1.0, 2^31 - 1) ... Afterwards the structure
    readers describe that compute, not an earlier one"; the files of lbmdem_write_structure are those of its own arguments in either
    order of the two writers (what lbmdem_run_scene does at a DEM event with both outputs on)"""
    with Stack(pkg, tmp_path, tag="q2:") as h:
        ws, wv = o("write_structure", p=gs.WRITE_STRUCTURE), o("write_voronoi", rcut=gs.WRITE_VORONOI)
        run_all(h, [gs.RESET, ws, wv])
        assert h.model.expect("structure", "lbmdem_download_structure_hist").result["nbins"] == 1
        run_all(h, [ws])
        assert h.model.expect("voronoi", "lbmdem_download_voronoi_faces").result["rcut"] == gs.WRITE_VORONOI
        assert h.model.expect("structure", "lbmdem_download_structure_hist").result["nbins"] == gs.WRITE_STRUCTURE[1]
        run_all(h, [wv, o("structure", p=SC), wv])


def test_q3_the_contact_export_between_a_cluster_compute_and_its_readers(pkg, tmp_path):
    """Force chains: "No call of the contact export (lbmdem_contact_stats, lbmdem_download_contacts with any room,
    lbmdem_write_contacts) changes a cluster result", and lbmdem_write_clusters writes "the records of its own compute": the cluster
    files and DEM%.6i_clusters.ps are those of the compute they belong to (the harness compares the four files)"""
    with Stack(pkg, tmp_path, tag="q3:") as h:
        run_all(h, [gs.RESET, o("clusters", p=P0)])
        for room in gs.ROOMS:
            run_all(h, [o("download_contacts", room=room), o("write_clusters", p=gs.WRITE_CLUSTERS)])
        run_all(h, [o("write_contacts"), o("clusters", p=P1), o("write_contacts"), o("write_clusters", p=P0),
                    o("download_contacts", room="short"), o("write_clusters", p=P1)])
        # the records grow: a table sub-step from the moved kinematics, then the same again
        run_all(h, [o("upload_moved"), o("table_substep"), o("write_clusters", p=P1), o("download_contacts", room="zero"),
                    o("clusters", p=P0), o("download_contacts", room="enough")])


def test_q4_refused_computes(pkg, tmp_path):
    """Voronoi cells: "A refused lbmdem_voronoi_compute (no valid list, a counts-only list) discards an earlier result: the readers
    are refused until the next compute that succeeds". Force chains: "A compute that is refused for fmin or zmin changes nothing:
    an earlier result stays readable; one that is refused because the contact records are not valid finds the readers refused
    already\""""
    with Stack(pkg, tmp_path, tag="q4:") as h:
        run_all(h, [gs.RESET, o("clusters", p=P0), o("structure", p=S0), o("voronoi"), o("clusters", p=(-1.0, True, 2))])
        assert h.model.expect("clusters", "lbmdem_download_clusters").result["p"] == P0
        with pytest.raises(pkg.LbmDemError, match="zmin must lie in 0 .. 6"):
            h.sim.clusters(1.0, True, 7)
        h.check_all()
        run_all(h, [o("structure", p=SC), o("voronoi")])          # counts only: refused, and the cells of S0 are gone
        assert h.model.expect("voronoi", "lbmdem_download_voronoi_faces").state == "refuses"
        run_all(h, [o("structure", p=S1), o("voronoi"), o("dem_substep"), o("voronoi"), o("clusters", p=P0)])          # a stale list


def test_q5_a_fluid_step_alone_leaves_the_grain_stages_readable(pkg, tmp_path):
    """The contact network export: "A fluid step alone (lbmdem_lbm_step), lbmdem_upload_f, the coarse-grained and the flow fields
    move no grain and no wall: the contact export, the clusters, the structure and the Voronoi readers go on answering" -- while
    the coarse fields, which read the populations, change"""
    with Stack(pkg, tmp_path, tag="q5:") as h:
        run_all(h, [gs.RESET, o("clusters", p=P0), o("structure", p=S0), o("voronoi")])
        before = h.sim.coarse_fields(*gs.COARSE[0])[0]
        run_all(h, [o("lbm_step"), o("coarse", cell=gs.COARSE[0]), o("lbm_step"), o("upload_f"), o("flow")])
        assert gs.co.mismatches(h.sim.coarse_fields(*gs.COARSE[0])[0], before)
        for stage, who in gs.ALL_READERS:
            assert h.model.expect(stage, who).state == "answers"


BETWEEN = (o("coarse", cell=gs.COARSE[0]), o("flow"), o("coarse", cell=gs.COARSE[1]))


@pytest.mark.parametrize("between", BETWEEN, ids=[gs.show(b).replace(" ", "") for b in BETWEEN])
def test_q6_coarse_and_flow_between_any_two(pkg, tmp_path, between):
    """the same sentence: the coarse and the flow fields keep no result and have scratch of their own; between every ordered pair
    of operations on the four stateful stages, the coarse fields at either cell size (the staging grows) or the flow fields: no
    other stage's result changes. One case per operation in between, each over all 72 pairs"""
    stateful = [op_ for s in gs.STAGES for op_ in gs.TWO_EACH[s]] + [o("structure", p=SC)]
    with Stack(pkg, tmp_path, tag="q6:") as h:
        h.run(gs.RESET)
        for a, b in itertools.permutations(stateful, 2):
            run_all(h, [a, between, b], check=False)
            h.check_all()
        assert sum(op_ == between for op_ in h.done) == 72


def test_the_device_views(pkg, tmp_path):
    """cluster_grains_tensors, voronoi_tensors and structure_tensors after an interleaved sequence: they equal the downloads and are
    refused when the downloads are"""
    names = dict(clusters="lbmdem_cluster_grains_device", structure="lbmdem_structure_grains_device",
                 voronoi="lbmdem_voronoi_grains_device")
    with Stack(pkg, tmp_path, tag="views:") as h:
        sim = h.sim
        views = dict(clusters=(sim.cluster_grains_tensors, sim.cluster_grains), structure=(sim.structure_tensors, sim.structure_grains),
                     voronoi=(sim.voronoi_tensors, sim.voronoi_grains))
        for op_ in [gs.RESET, o("structure", p=S1), o("clusters", p=P0), o("voronoi"), o("structure", p=S0), o("clusters", p=P1),
                    o("coarse", cell=gs.COARSE[1]), o("write_voronoi", rcut=gs.WRITE_VORONOI), o("structure", p=SC), o("move_walls_other"),
                    o("table_substep"), o("clusters", p=P0), o("structure", p=S0), o("voronoi"), o("upload_same")]:
            h.run(op_)
            h.check_all()
            for stage, (view, download) in views.items():
                e = h.model.expect(stage, names[stage].replace("_device", "").replace("lbmdem_", "lbmdem_download_"))
                if e.state == "refuses":
                    h.refused(view, e.sentence.replace(e.sentence.split(":")[0], names[stage]), names[stage])
                    continue
                tv, g = view(), download()
                for name in tv:
                    assert tv[name].is_cuda and np.array_equal(tv[name].cpu().numpy().view(np.uint8),
                                                               np.ascontiguousarray(g[name]).view(np.uint8)), (h.where(), stage, name)
                del tv


# ---- all five outputs at once: lbmdem_run_scene and the host driver on G6 ----

REF_DIR = os.path.join(gs.cu.HERE, "golden", "dem_G6_4000steps")
EXE = os.path.join(os.path.dirname(gs.cu.HERE), "2d-lbm-dem_amd", "host", "lbmdem")
FILES = dict(contacts=("contacts000000.dat", "DEM000000_chains.ps"),
             clusters=("clusters000000.dat", "cluster_table000000.dat", "DEM000000_clusters.ps", "clusters.data"),
             structure=("structure000000.dat", "gr000000.dat", "structure.data"), voronoi=("voronoi000000.dat", "voronoi.data"),
             coarse=("coarse000000.dat",))
G6_CLUSTERS, G6_CLUSTERS_ABS, G6_BINS, G6_SHELL, G6_COARSE = (0.5, True, 3), (0.0, False, 1), 32, 1.2, (16, 8)


def g6_setters(sim, z, clusters=G6_CLUSTERS):
    """the five setters by name; the structure's R1 = 3.3 and the Voronoi's R2 = 2.2 mean diameters"""
    D = 2.0 * float(np.mean(z["r_mm"] * 1e-3))
    return dict(contacts=lambda: sim.set_contacts_output(True), clusters=lambda: sim.set_clusters_output(True, *clusters),
                structure=lambda: sim.set_structure_output(True, 3.3 * D, G6_BINS, G6_SHELL),
                voronoi=lambda: sim.set_voronoi_output(True, 2.2 * D), coarse=lambda: sim.set_coarse_output(*G6_COARSE)), D


@pytest.fixture(scope="module")
def g6(pkg, tmp_path_factory):
    """the G6 golden through run_scene to step 4000 (the single stages' test_g6_at_4000_through_run_scene): plain, with each of the
    five outputs alone, with all five, with all five set in reverse order, and with the absolute cluster threshold"""
    z = np.load(os.path.join(REF_DIR, "inputs_and_table.npz"))
    r, x, y = z["r_mm"] * 1e-3, z["x_mm"] * 1e-3, z["y_mm"] * 1e-3
    dirs, ends = {}, {}

    def run(name, which, clusters=G6_CLUSTERS):
        dirs[name] = tmp_path_factory.mktemp(name)
        with pkg.LbmDem(256, 200, r, x, y) as sim:
            setters, _ = g6_setters(sim, z, clusters)
            for w in which:
                setters[w]()
            sim.run_scene(4000, str(dirs[name]))
            ends[name] = {what: getattr(sim, what) for what in ("f", "obst", "kinematics", "fhf")}
    run("plain", ())
    for name in FILES:
        run(name, (name,))
    run("all", tuple(FILES))
    run("reversed", tuple(FILES)[::-1])
    run("abs", tuple(FILES), G6_CLUSTERS_ABS)
    run("clusters_abs", ("clusters",), G6_CLUSTERS_ABS)
    return dict(z=z, dirs=dirs, ends=ends)


def test_run_scene_with_all_five_outputs(g6):
    """every file of a DEM event with contacts, clusters, structure (R1), Voronoi (R2 != R1) and coarse outputs on is byte-equal to
    what the same scene writes with that output alone, in either order of the setters; the plain run's files and the final state are
    untouched"""
    dirs, ends = g6["dirs"], g6["ends"]
    plain = sorted(os.listdir(dirs["plain"]))
    assert "DEM000000.dat" in plain
    for name in ("all", "reversed"):
        assert sorted(os.listdir(dirs[name])) == sorted(plain + [f for fs in FILES.values() for f in fs]), name
        for f in plain:
            assert (dirs[name] / f).read_bytes() == (dirs["plain"] / f).read_bytes(), (name, f)
        for alone, files in FILES.items():
            assert sorted(os.listdir(dirs[alone])) == sorted(plain + list(files)), alone
            for f in files:
                assert (dirs[name] / f).read_bytes() == (dirs[alone] / f).read_bytes(), (name, f)
        for what, v in ends["plain"].items():
            assert np.array_equal(ends[name][what], v), (name, what)
    # the two cutoffs do differ, and so do the two cluster parametrisations
    D = g6_setters(None, g6["z"])[1]
    assert (dirs["all"] / "voronoi000000.dat").read_text().splitlines()[0] == "# rcut %e" % (2.2 * D) != "# rcut %e" % (3.3 * D)
    assert (dirs["all"] / "structure000000.dat").read_text().splitlines()[0] == "# rcut %e nbins %d shell %e" % (3.3 * D, G6_BINS, G6_SHELL)
    for f in FILES["clusters"]:
        assert (dirs["abs"] / f).read_bytes() == (dirs["clusters_abs"] / f).read_bytes() != (dirs["all"] / f).read_bytes(), f


@pytest.mark.parametrize("absolute", [False, True], ids=["relative", "absolute"])
def test_host_driver_with_all_five_outputs(po, g6, tmp_path, absolute):
    """`lbmdem <G6> --contacts --clusters K --clusters-zmin Z --structure R1 --voronoi R2 --coarse CWxCH` (and with --clusters-abs F)
    in a child process: run_scene's files with the matching setters, byte for byte"""
    z = g6["z"]
    D = g6_setters(None, z)[1]
    sample = tmp_path / "packing.data"
    po.write_sample(str(sample), z["r_mm"], z["x_mm"], z["y_mm"])
    p = G6_CLUSTERS_ABS if absolute else G6_CLUSTERS
    flags = ["--contacts"] + (["--clusters-abs", repr(p[0])] if absolute else ["--clusters", repr(p[0])]) + [
        "--clusters-zmin", str(p[2]), "--structure", repr(3.3 * D), "--structure-bins", str(G6_BINS), "--structure-shell", repr(G6_SHELL),
        "--voronoi", repr(2.2 * D), "--coarse", "%dx%d" % G6_COARSE]
    out = subprocess.run([EXE, str(sample), "--lx", "256", "--ly", "200", "--steps", "4001"] + flags, capture_output=True, text=True,
                         cwd=tmp_path, timeout=600)
    assert out.returncode == 0, out.stderr[-600:]
    want = g6["dirs"]["abs" if absolute else "all"]
    for files in FILES.values():
        for f in files:
            assert (tmp_path / f).read_bytes() == (want / f).read_bytes(), f
