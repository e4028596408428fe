"""CPU: the harness of tests/test_gpu_pore_stack.py pinned before it is trusted (tests/pore_stack_util.py): the single stages'
restatements agree where they overlap on every map of the menu, the pair list is complete, and the committed walks reach what they
are there for -- asserted on the model alone, so that a later edit to the menu cannot silently lose it."""
import itertools

import numpy as np
import pytest

import clearance_util as cz
import drainage_util as du
import geodesic_util as gu
import netflux_util as fu
import netsolve_util as su
import network_util as nu
import pore_stack_util as ps
import pore_util as pz

LX, LY, N = ps.LX, ps.LY, 7


def the_map(name):
    """the handle's map is stood in for by a packing of random discs, as in the single stages' host tests"""
    return du.random_discs(LX, LY, N, 4850) if name in (ps.OWN, "own_copy") else ps.callers_map(name, LX, LY, N)


@pytest.fixture(scope="module")
def f():
    return np.random.default_rng(48).uniform(0.01, 0.5, (LX, LY, 9))


def rows_equal(a, b):
    return a.dtype == b.dtype and len(a) == len(b) and all(np.array_equal(a[k], b[k]) for k in a.dtype.names)


@pytest.mark.parametrize("name", [m for m in ps.MAPS if m != "own_copy"])
def test_the_restatements_agree_where_they_overlap(name, f):
    M = the_map(name)
    C = cz.restate(M, N)
    nets = {merge: nu.restate(M, N, merge) for merge in ps.MENU["network"]["merge"]}
    for net in nets.values():          # the network's d2 is the clearance's; level 0 does not know the merge
        assert np.array_equal(net["d2"], C["d2"]) and rows_equal(net["links0"], nets[-1]["links0"])
        assert np.array_equal(net["body"], nets[-1]["body"])
    # drainage: the network's bodies and level-0 links (its own network, not one handed in), the clearance's histogram
    for sides in ps.SIDES:
        D = du.restate(M, N, *sides)
        assert len(D["A"]) == len(nets[-1]["bodies"]) and len(D["passes"]) == len(nets[-1]["links0"])
        assert rows_equal(D["network"]["links0"], nets[-1]["links0"]) and len(D["hist"]) == len(C["hist"])
        assert D["hist"].sum() == C["hist"].sum() == C["counts"]["fluid_nodes"] == D["counts"]["fluid_nodes"]
    D = du.restate(M, N, 15, max(LX, LY), 0)          # every fluid node an inlet: access is d2, bin for bin
    assert np.array_equal(D["access"], C["d2"]) and np.array_equal(D["hist"], C["hist"])
    # netflux and netsolve: the link table of (merge, level) is the network's, and so are the regions
    for merge, level in itertools.product(ps.MENU["netflux"]["merge"], ps.MENU["netflux"]["level"]):
        table = nets[merge]["links1" if level else "links0"]
        regions = len(nets[merge]["groups" if level else "bodies"])
        F = fu.restate(M, f, N, merge, level)
        assert rows_equal(F["table"], table) and len(F["links"]) == len(table) and len(F["regions"]) == regions
        assert np.array_equal(F["links"]["edges"], table["edges"])
        for sides in ps.SIDES:
            S = su.restate(M, N, *sides, merge, level)
            assert rows_equal(S["table"], table) and len(S["links"]) == len(table) and len(S["regions"]) == regions
            assert S["counts"]["regions"] == F["counts"]["regions"] and S["counts"]["links"] == F["counts"]["links"]
    # geodesic with min_d2 = 4 passes exactly the nodes with d2 >= 4 of the clearance's plane
    assert np.array_equal(gu.passable(M, N, 4)[1], C["d2"] >= 4)
    for sides in ps.SIDES:
        G = gu.restate(M, N, *sides, 8, 4)
        assert G["counts"]["passable_nodes"] == int((C["d2"] >= 4).sum()) and G["counts"]["fluid_nodes"] == C["counts"]["fluid_nodes"]
        assert np.array_equal(G["dist"] >= 0, (G["dist"] >= 0) & (C["d2"] >= 4))
    # the two extremes: the counts the single stages' tests assert
    P = pz.restate(M, f, N, 8)
    if name == "no_fluid":
        assert P["counts"]["components"] == 0 and P["counts"]["largest_label"] == -1 and C["counts"]["fluid_nodes"] == 0
        assert nets[-1]["counts"]["bodies"] == 0 and len(D["A"]) == 0
        assert fu.restate(M, f, N, -1, 0)["counts"] == dict(zip(fu.NETFLUX_COUNTERS, (0, 0, 0, 0, 0, 0, 0, 0, -1, 0)))
        assert su.restate(M, N, *ps.SIDES[0], -1, 0)["counts"]["regions"] == 0
        assert gu.restate(M, N, *ps.SIDES[0])["counts"]["passable_nodes"] == 0
    if name == "all_fluid":
        assert P["counts"]["components"] == 1 and P["counts"]["spanning"] == 3 and P["counts"]["largest_nodes"] == LX * LY
        assert nets[0]["counts"]["bodies"] == 1 and nets[0]["counts"]["body_links"] == 0
        assert su.restate(M, N, *ps.SIDES[0], 0, 1)["counts"] == dict(zip(su.NETSOLVE_COUNTERS, (1, 0, 1, 0, 1, 0, 0, 0, 0, -1)))
        c = fu.restate(M, f, N, 0, 1)["counts"]
        assert c["regions"] == 1 and c["links"] == 0 and c["strongest_link"] == -1
        assert c["edges"] == LX * (LY - 1) + (LX - 1) * LY + 2 * (LX - 1) * (LY - 1)
        assert D["counts"]["reached_nodes"] == LX * LY and gu.restate(M, N, T_, 4, B_)["counts"]["shortest"] == 215


T_, B_ = ps.T, ps.B


def regions_of(name):
    """the regions of the finest level of a map of the menu: the bodies of its network"""
    return nu.restate(the_map(name), N, -1)["counts"]["bodies"]


def test_the_maps_differ_widely_in_size():
    sizes = {m: regions_of(m) for m in ps.MAPS if m != "own_copy"}
    assert sizes["no_fluid"] == 0 and sizes["all_fluid"] == 1 and sizes["chambers"] > 100, sizes
    assert nu.restate(the_map("chambers"), N, -1)["counts"]["body_links"] > 100


def test_the_operation_list():
    ops = ps.operations()
    assert len(set(ops)) == len(ops) and {o.kind for o in ops} == set(ps.STAGES) | set(ps.STEPS)
    for stage in ps.STAGES:
        mine = [o for o in ops if o.kind == stage]
        assert {o.map for o in mine} == set(ps.MAPS)
        for name, values in ps.MENU[stage].items():
            assert {dict(o.params)[name] for o in mine} == set(values), (stage, name)
    for seed in ps.SEEDS:
        assert set(ps.walk(seed)) <= set(ops) and len(ps.walk(seed)) == ps.WALK_LENGTH and ps.walk(seed) == ps.walk(seed)
    assert len({tuple(ps.walk(seed)) for seed in ps.SEEDS}) == len(ps.SEEDS) == 3


def test_the_pair_list_is_complete():
    cases = ps.pair_cases()
    assert len(cases) == 14 and set(cases) == {(s, own) for s in ps.STAGES for own in (True, False)}
    for agree in (True, False):
        got = ps.pairs(agree)
        assert len(got) == 14 * 14
        seen = {((a.kind, a.map == ps.OWN), (b.kind, b.map == ps.OWN)) for a, b in got}
        assert seen == set(itertools.product(cases, cases))
        assert all(a in ps.operations() and b in ps.operations() for a, b in got)
        # the members that share the network agree in merge in the one parametrisation and differ in the other
        for a, b in got:
            ma = -1 if a.kind == "drainage" else dict(a.params).get("merge")
            mb = -1 if b.kind == "drainage" else dict(b.params).get("merge")
            if ma is not None and mb is not None and not a.kind == b.kind == "drainage":          # (which has no merge to differ in)
                assert (ma == mb) == agree, (a, b)
            if a.map != ps.OWN and b.map != ps.OWN:
                assert a.map != b.map
    assert len(set(itertools.permutations(ps.TWO_MERGES))) == 24
    assert {(o.kind, dict(o.params).get("merge")) for o in ps.TWO_MERGES} == {("netflux", 1), ("netsolve", -1), ("drainage", None), ("network", 0)}


def test_the_model_on_the_cases_the_single_stages_pin():
    """the sentences of the header that the single stages' tests already hold the device to, held to the model"""
    own = lambda stage, **p: ps.compute(stage, **p)
    last = lambda ops: {s: e.state for s, e in ps.trace(ops)[-1].items()}
    sides = ps.SIDES[0]
    assert set(last([ps.step("lbm_step")]).values()) == {"refuses"}
    # a later network() takes the tables away (test_gpu_netsolve, test_gpu_netflux, test_gpu_drainage)
    for stage, p in (("netsolve", dict(sides=sides, merge=-1, level=0)), ("netflux", dict(merge=-1, level=0)), ("drainage", dict(sides=sides))):
        got = last([own(stage, **p)])
        assert got[stage] == got["network"] == got["clearance"] == "answers" and got["pores"] == got["geodesic"] == "refuses"
        assert last([own(stage, **p), own("network", merge=-1)])[stage] == "refuses"
        for kind in ps.STEPS:
            assert set(last([own(stage, **p), ps.step(kind)]).values()) == {"refuses"}
    # a reused network keeps its readers and its other readers' rows
    got = last([own("netflux", merge=1, level=1), own("netsolve", sides=sides, merge=1, level=0), own("drainage", sides=sides)])
    assert got["netflux"] == got["netsolve"] == got["drainage"] == "answers"
    got = ps.trace([own("netflux", merge=1, level=1), own("netsolve", sides=sides, merge=0, level=0)])[-1]
    assert got["netflux"].state == "refuses" and got["netflux"].why.kind == "netsolve" and got["network"].result["params"] == dict(merge=0)
    # a caller's map is never reused, and takes the handle's upstream results with it
    got = ps.trace([own("network", merge=-1), ps.compute("drainage", "two_pores", sides=sides), own("drainage", sides=sides)])
    assert got[1]["network"].result["map"] == got[1]["clearance"].result["map"] == "two_pores"
    assert got[2]["network"].result["map"] == ps.OWN and got[2]["network"].result["op"].kind == "drainage"
    # the geodesic over the handle's map and min_d2 > 1 goes with the clearance it was made over; any other stays
    for m, min_d2, want in ((ps.OWN, 4, "refuses"), (ps.OWN, 0, "answers"), ("two_pores", 4, "answers")):
        g = ps.compute("geodesic", m, sides=sides, conn=8, min_d2=min_d2)
        assert last([g, own("clearance")])["geodesic"] == want
        assert last([g, ps.compute("network", "chambers", merge=0)])["geodesic"] == want
        assert last([own("clearance"), g, own("network", merge=0)])["geodesic"] == "answers"          # (the clearance is reused)
    assert last([ps.compute("geodesic", sides=sides, conn=8, min_d2=0)])["clearance"] == "refuses"
    assert last([ps.compute("geodesic", sides=sides, conn=8, min_d2=4)])["clearance"] == "answers"
    assert ps.EITHER == ()


@pytest.mark.parametrize("seed", ps.SEEDS)
def test_the_walks_reach_what_they_are_there_for(seed):
    ops = ps.walk(seed)
    seen = ps.trace(ops)
    answered_by_another, refused_by_a_sibling = set(), set()
    answers = checks = 0
    for op, after in zip(ops, seen):
        for stage, e in after.items():
            checks += 1
            answers += e.state == "answers"
            if e.state == "answers" and stage != op.kind:
                answered_by_another.add(stage)
            if e.state == "refuses" and isinstance(e.why, ps.Op) and e.why.kind in ps.STAGES:
                refused_by_a_sibling.add(stage)
    assert answered_by_another == set(ps.STAGES), sorted(set(ps.STAGES) - answered_by_another)
    assert refused_by_a_sibling >= set(ps.DOWNSTREAM), sorted(set(ps.DOWNSTREAM) - refused_by_a_sibling)
    # the tables shrink to (next to) nothing under a sibling's valid result and grow again
    size = {m: regions_of(m) for m in ps.MAPS if m != "own_copy"}
    size["own_copy"] = size[ps.OWN]
    maps = [op.map for op in ops if op.kind in ("network", "drainage", "netflux", "netsolve")]
    down = any(size[a] > 100 and size[b] <= 1 for a, b in zip(maps, maps[1:]))
    up = any(size[a] <= 1 and size[b] > 100 for a, b in zip(maps, maps[1:]))
    assert down and up, (seed, maps)
    assert any(op.kind in ps.STEPS for op in ops)
    # not by refusing everything: at least a third of all reader checks expect an answer
    assert 3 * answers >= checks, (seed, answers, checks)
