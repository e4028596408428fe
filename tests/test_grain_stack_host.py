"""CPU: the harness of tests/test_gpu_grain_stack.py pinned before it is trusted (tests/grain_stack_util.py): the single stages'
restatements agree where one is made of another's output, the model decides every reader after every ordered pair of operations,
the committed walks reach what they are there for, and the inequalities that give the device comparisons their teeth hold on the
restatements alone -- so that a GPU test can never pass because two answers coincide. No device is touched."""
import collections
import itertools

import numpy as np
import pytest

import cluster_util as cl
import coarse_util as co
import contacts_util as cu
import grain_stack_util as gs
import moving_walls_util as mw
import voronoi_util as vu

SENTENCES = (gs.NO_TABLE, gs.WALL_MOVED, gs.NO_CLUSTERS, gs.NO_STRUCTURE, gs.COUNTS_ONLY, gs.NO_VORONOI)


@pytest.fixture(scope="module")
def S(pkg):
    """the scene, its walls as a new handle has them (dtt = 1 s: the lattice's edge), and the restated records of the table sub-step
    that starts from the base and from the moved kinematics, over the list of all pairs with every wall a candidate"""
    lx, ly, r, k = gs.scene()
    cfg = pkg.derive(lx, ly, r, physics=gs.physics(pkg, lx, ly, r))
    box = (cfg.Mgx, cfg.Mdx, cfg.Mby, cfg.Mhy)
    assert box == (0.0, 1e-3 * lx / 10, 0.0, 1e-3 * ly / 10)
    P = cu.params_of_config(cfg)

    def records(kin, Mgx=box[0]):
        return cu.restate(kin, r, gs.all_pairs(len(r)), np.full(len(r), 15, np.int32), dict(P, Mgx=Mgx), False)[0]
    return dict(lx=lx, ly=ly, r=r, k=k, box=box, D=gs.mean_diameter(r), records=records, dx=cfg.dx)


def test_the_scene_touches_three_walls(S):
    rec = S["records"](S["k"])
    walls = collections.Counter(int(j) for j in rec["j"] if j < 0)
    assert walls[cu.WALL_L] == 1 and walls[cu.WALL_R] == 1 and walls[cu.WALL_B] >= 3 and walls[cu.WALL_T] == 0, walls
    assert len(S["r"]) == 65 and (rec["j"] >= 0).sum() >= 65 // 8
    # no grain lies deeper in a wall or in a neighbour than a packing under its own weight does: the steps stay tame
    assert rec["dn"].min() > -5e-6, rec["dn"].min()


def test_the_clusters_restatement_over_the_contacts_restatements_records(S):
    rec, n = S["records"](S["k"]), len(S["r"])
    x, y = S["k"][:, 0], S["k"][:, 1]
    for p in gs.CLUSTER_PARAMS + (gs.WRITE_CLUSTERS,):
        R = cl.restate(rec, n, x, y, *p)
        c = R["counts"]
        sel = rec["fn"] >= R["thr"]
        assert c["selected_pairs"] == int((sel & (rec["j"] >= 0)).sum()) and c["selected_walls"] == int((sel & (rec["j"] < 0)).sum())
        assert R["degree"].sum() == 2 * c["selected_pairs"] + c["selected_walls"]
        assert c["clusters"] == len(R["table"]) and int(R["table"]["contacts"].sum()) == c["selected_pairs"]
        assert (R["label"] <= np.arange(n)).all() and (R["label"][R["label"]] == R["label"]).all()
        wall_bits = np.zeros(n, np.int32)
        for rcd in rec[sel & (rec["j"] < 0)]:
            wall_bits[rcd["i"]] |= 1 << (-int(rcd["j"]) - 1)
        assert np.array_equal(R["walls"], wall_bits)
    # absolute 0 selects every record with fn >= 0: the left and the bottom wall's (the right wall's fn is <= 0 by the reference)
    R = cl.restate(rec, n, x, y, *gs.CLUSTER_PARAMS[1])
    assert (np.bitwise_or.reduce(R["walls"]) & 5) == 5


def test_the_voronoi_restatement_over_the_structure_restatements_list(S):
    x, y, r, D = S["k"][:, 0], S["k"][:, 1], S["r"], S["D"]
    for p in gs.STRUCTURE_PARAMS[:2] + ((gs.WRITE_VORONOI, 1, 1.0, True),):
        rcut = p[0] * D
        L = gs.structure_restatement(x, y, r, rcut, p[1], p[2])
        V = gs.voronoi_restatement(x, y, r, S["box"], rcut)
        assert L["counts"]["entries"] == len(L["nbr"]) == int(L["hist"].sum()) * 2
        for i in range(len(r)):          # a cell's grain faces are among the list's neighbours of that grain, each once
            faces = V["fsrc"][V["foff"][i]:V["foff"][i + 1]]
            mine = set(L["nbr"][L["offsets"][i]:L["offsets"][i + 1]].tolist())
            grains = [int(j) for j in faces if j >= 0]
            assert set(grains) <= mine and len(set(grains)) == len(grains) == V["grains"]["faces"][i], i
        assert V["counts"]["cells"] == len(r) and V["counts"]["overflowed"] == 0
        # the cells tile the box where every cell is complete: the widest cutoff's areas add up to W * H within n eps W H
        if V["counts"]["complete"] == len(r):
            area = (S["box"][1] - S["box"][0]) * (S["box"][3] - S["box"][2])
            assert abs(float(V["grains"]["area"].sum()) - area) <= len(r) * np.finfo(float).eps * area
    assert (V["grains"]["walls"] > 0).sum() >= 4


def test_the_comparisons_have_teeth(S):
    x, y, r, D, box = S["k"][:, 0], S["k"][:, 1], S["r"], S["D"], S["box"]
    # the two structure parametrisations (and the writers' own) give different lists AND different cells
    cuts = [gs.STRUCTURE_PARAMS[0], gs.STRUCTURE_PARAMS[1], gs.WRITE_STRUCTURE + (True,), (gs.WRITE_VORONOI, 1, 1.0, True)]
    for a, b in itertools.combinations(cuts, 2):
        La, Lb = (gs.structure_restatement(x, y, r, p[0] * D, p[1], p[2]) for p in (a, b))
        assert len(La["nbr"]) != len(Lb["nbr"]) and len(La["hist"]) != len(Lb["hist"]), (a, b)
        assert La["grains"].tobytes() != Lb["grains"].tobytes()
        Va, Vb = (gs.voronoi_restatement(x, y, r, box, p[0] * D) for p in (a, b))
        assert len(mw.records_that_differ(Va, Vb)) >= 5, (a, b)
    counts_only = gs.STRUCTURE_PARAMS[2]
    assert not counts_only[3] and all(counts_only[0] != p[0] and counts_only[1] != p[1] for p in cuts)
    # the cluster parametrisations give different labels, cores and tables
    rec, n = S["records"](S["k"]), len(r)
    for a, b in itertools.combinations(gs.CLUSTER_PARAMS + (gs.WRITE_CLUSTERS,), 2):
        Ra, Rb = (cl.restate(rec, n, x, y, *p) for p in (a, b))
        assert not np.array_equal(Ra["label"], Rb["label"]) and not np.array_equal(Ra["core"], Rb["core"]), (a, b)
        assert not cl.same_table(Ra["table"], Rb["table"]) and Ra["counts"] != Rb["counts"]
    # the moved kinematics change a contact record, a neighbour entry and a cell; moving twice is not moving once
    k1, k2 = gs.moved(S["k"]), gs.moved(S["k"], 2)
    assert not cu.same_records(S["records"](S["k"]), S["records"](k1)) and not cu.same_records(S["records"](k1), S["records"](k2))
    for ka, kb in ((S["k"], k1), (k1, k2)):
        for p in cuts[:2]:
            La, Lb = (gs.structure_restatement(k[:, 0], k[:, 1], r, p[0] * D, p[1], p[2]) for k in (ka, kb))
            Va, Vb = (gs.voronoi_restatement(k[:, 0], k[:, 1], r, box, p[0] * D) for k in (ka, kb))
            assert La["grains"].tobytes() != Lb["grains"].tobytes() and len(mw.records_that_differ(Va, Vb)) >= 1
        La, Lb = (gs.structure_restatement(k[:, 0], k[:, 1], r, cuts[1][0] * D, 16, 1.0) for k in (ka, kb))
        assert not np.array_equal(La["nbr"], Lb["nbr"])
    # a side wall AMP * sin(1) further: another left-wall record, other cells
    shift = gs.AMP * np.sin(1.0)
    assert not cu.same_records(S["records"](S["k"]), S["records"](S["k"], Mgx=shift))
    moved_box = (box[0] + shift, box[1] + shift, box[2], box[3])
    assert len(mw.records_that_differ(gs.voronoi_restatement(x, y, r, box, cuts[0][0] * D),
                                      gs.voronoi_restatement(x, y, r, moved_box, cuts[0][0] * D))) >= 2
    # the two coarse grids differ
    assert len({co.grid(S["lx"], S["ly"], *c) for c in gs.COARSE}) == 2


def test_the_operation_list():
    ops = gs.operations()
    assert len(set(ops)) == len(ops) == 28 and {o.kind for o in ops} == set(gs.STEPS) | set(gs.COMPUTES)
    assert set(gs.operations(True)) | set(gs.operations(False)) == set(ops)
    assert len(gs.operations(True)) == len(gs.operations(False)) == 27
    for seed in gs.SEEDS:
        shaking = seed != gs.STILL_SEED
        assert set(gs.walk(seed)) <= set(gs.operations(shaking)) and len(gs.walk(seed)) == gs.WALK_LENGTH and gs.walk(seed) == gs.walk(seed)
    assert len({tuple(gs.walk(seed)) for seed in gs.SEEDS}) == len(gs.SEEDS) == 3 and gs.STILL_SEED in gs.SEEDS
    assert len(list(itertools.permutations(gs.STAGES))) == 24 and all(len(gs.TWO_EACH[s]) == 2 for s in gs.STAGES)


def decided(e, who):
    """an Expect names the compute a reader answers with, or one of the stages' sentences"""
    if e.state == "answers":
        return isinstance(e.result, dict) and ("table" in e.result or isinstance(e.result.get("op"), gs.Op))
    return e.state == "refuses" and e.sentence in [s % who for s in SENTENCES]


@pytest.mark.parametrize("shaking", [True, False], ids=["shaking", "still"])
@pytest.mark.parametrize("state", sorted(gs.STATES))
def test_the_model_decides_every_reader_after_every_ordered_pair(state, shaking):
    pairs = gs.pairs(shaking)
    assert len(pairs) == 27 * 27 and len(set(pairs)) == len(pairs)
    outcomes = collections.Counter()
    for a, b in pairs:
        for after in gs.trace([a, b], shaking, prepare=(gs.RESET,) + gs.STATES[state]):
            for (stage, who), e in after.items():
                assert decided(e, who), (state, gs.show(a), gs.show(b), who, e)
                outcomes[stage, e.state] += 1
    assert gs.EITHER == ()
    for stage in gs.STAGES:          # neither everything answers nor everything refuses
        assert outcomes[stage, "answers"] > 100 and outcomes[stage, "refuses"] > 100, outcomes


def test_the_model_on_the_cases_the_single_stages_pin():
    """the sentences of the header that the single stages' tests already hold the device to, held to the model"""
    o = gs.op
    P0, S0, SC = gs.CLUSTER_PARAMS[0], gs.STRUCTURE_PARAMS[0], gs.STRUCTURE_PARAMS[2]

    def last(ops, shaking=True):
        return {who: (e.state, e.sentence) for (_, who), e in gs.trace(ops, shaking)[-1].items()}
    every = [o("clusters", p=P0), o("structure", p=S0), o("voronoi")]
    assert {s for s, _ in last(every).values()} == {"answers"}
    for step in ("dem_substep", "renderScene", "upload_same", "upload_moved"):          # test_validity, ..._after_a_move
        got = last(every + [o(step)])
        assert {s for s, _ in got.values()} == {"refuses"}
        assert got["lbmdem_download_contacts"][1] == gs.NO_TABLE % "lbmdem_download_contacts"
    got = last(every + [o("table_substep")])          # another table sub-step: the results were the last one's
    assert got["lbmdem_download_contacts"][0] == "answers" and got["lbmdem_download_clusters"][0] == "refuses"
    got = last(every + [o("rebuild")])          # (no wall has moved: the Voronoi cells stay, test_gpu_moving_walls)
    assert got["lbmdem_contact_stats"] == ("refuses", gs.NO_TABLE % "lbmdem_contact_stats")
    assert got["lbmdem_download_voronoi_faces"][0] == got["lbmdem_download_structure_hist"][0] == "answers"
    got = last(every + [o("move_walls_other")])          # test_gpu_moving_walls: the guards
    assert got["lbmdem_download_contacts"] == ("refuses", gs.WALL_MOVED % "lbmdem_download_contacts")
    assert got["lbmdem_cluster_rounds"][0] == got["lbmdem_download_voronoi_grains"][0] == "refuses"
    assert got["lbmdem_download_structure_neighbours"][0] == "answers"
    got = last(every + [o("move_walls_other"), o("rebuild")])          # the rebuild discards Mdx's offset: a wall changes again
    assert got["lbmdem_download_contacts"] == ("refuses", gs.NO_TABLE % "lbmdem_download_contacts")
    assert {s for s, _ in last(every + [o("move_walls_same")], shaking=False).values()} == {"answers"}
    got = last(every + [o("structure", p=SC)])          # test_max_entries; the cells are the Voronoi stage's own
    assert got["lbmdem_download_structure_hist"][0] == "answers" and got["lbmdem_download_voronoi_faces"][0] == "answers"
    assert got["lbmdem_download_structure_grains"] == ("refuses", gs.COUNTS_ONLY % "lbmdem_download_structure_grains")
    after = gs.trace(every + [o("structure", p=gs.STRUCTURE_PARAMS[1])])[-1]          # ... of the rcut they were made with
    assert after["voronoi", "lbmdem_download_voronoi_faces"].result["rcut"] == S0[0]
    assert after["structure", "lbmdem_download_structure_hist"].result["rcut"] == gs.STRUCTURE_PARAMS[1][0]
    got = last(every + [o("structure", p=SC), o("voronoi")])          # a refused Voronoi compute discards the cells
    assert got["lbmdem_download_voronoi_faces"] == ("refuses", gs.NO_VORONOI % "lbmdem_download_voronoi_faces")
    got = last(every + [o("clusters", p=(-1.0, True, 2)), o("lbm_step"), o("upload_f"), o("flow"), o("coarse", cell=(8, 5))])
    assert {s for s, _ in got.values()} == {"answers"}          # a compute refused for fmin, a fluid step alone: nothing changes
    model = gs.Model(True)
    for op_ in [gs.RESET] + every + [o("write_voronoi", rcut=gs.WRITE_VORONOI)]:
        model.apply(op_)
    assert (model.st["rcut"], model.st["nbins"], model.st["shell"]) == (gs.WRITE_VORONOI, 1, 1.0) == (model.vo["rcut"], 1, 1.0)


def walk_census(seeds):
    ops_seen, answers, refusals = collections.Counter(), collections.Counter(), collections.Counter()
    worst = 0.0
    for seed in seeds:
        ops = gs.walk(seed)
        ops_seen.update(ops)
        mine = collections.Counter()
        for after in gs.trace(ops, seed != gs.STILL_SEED):
            for sw, e in after.items():
                (answers if e.state == "answers" else refusals)[sw] += 1
                mine[sw] += e.state == "refuses"
        worst = max(worst, max(mine.values()) / float(len(ops)))
    return ops_seen, answers, refusals, worst


def test_the_walks_reach_what_they_are_there_for():
    ops_seen, answers, refusals, worst = walk_census(gs.SEEDS)
    assert all(ops_seen[o] >= 2 for o in gs.operations()), [gs.show(o) for o in gs.operations() if ops_seen[o] < 2]
    for sw in gs.ALL_READERS:
        assert answers[sw] >= 5 and refusals[sw] >= 5, (sw, answers[sw], refusals[sw])
    # not by refusing everything: in no walk is a reader refused in more than 70 % of its calls
    assert worst <= 0.7, worst
    # every sentence occurs, and a reader answers with a compute another operation has made since
    said = {e.sentence.split(": ", 1)[1] for seed in gs.SEEDS for after in gs.trace(gs.walk(seed), seed != gs.STILL_SEED)
            for e in after.values() if e.state == "refuses"}
    assert said == {s.split(": ", 1)[1] for s in SENTENCES}, said
