"""The seven pore analyses as ONE chain (include/lbmdem_hip.h, "Pore space" through "Network pressures"): an operation list, a model
of which stage's readers must answer after any sequence of operations and with what, and the harness that holds a handle to it.

The stages share state: pores | clearance -> network -> drainage / netflux / netsolve, clearance -> geodesic (min_d2 > 1). A compute
may reuse its upstream's result or run the upstream itself, and a reader of a downstream stage is refused once the tables its rows
are aligned with have been rebuilt. The model below is written from the header's sentences, not from the guards in the .hip files;
the restatements it points to are the single stages' own (tests/*_util.py).

What the model encodes, each line with the sentence it comes from:
  network(map, merge)     reuses the clearance iff map is the handle's and there is a valid clearance result of the handle's map
                          ("with map == NULL and a clearance result of the handle's map that its guard still calls valid, that
                          result's d2 plane is reused"); otherwise it runs the clearance on the map, "and its readers are valid
                          afterwards as if the caller had called it".
  drainage(map, ..)       reuses the network iff map is the handle's and there are a valid network result and a valid clearance
                          result, both of the handle's map, "whatever merge that result was made with"; otherwise
                          lbmdem_network_compute(map, merge -1) runs.
  geodesic(map, min_d2)   min_d2 <= 1: "the clearance analysis is then neither needed nor run and its result, if there is one, is
                          not touched"; min_d2 > 1: the network's rule for the clearance.
  netflux, netsolve       reuse the network iff map is the handle's and there is a valid network result of the handle's map "made
                          with the same merge"; otherwise lbmdem_network_compute(map, merge) runs.
  readers                 all are refused until a compute has been made and after any step or sub-step; drainage's, netflux's and
                          netsolve's also "after a later lbmdem_network_compute", geodesic's "for a result made with min_d2 > 1 over
                          the handle's map, after a later lbmdem_clearance_compute" -- later computes that another stage runs
                          included, since those count "as if the caller had called".
A result over a caller's map stays readable until the next step: the handle's map has not changed since the compute."""
import collections
import hashlib
import random

import numpy as np

import clearance_util as cz
import drainage_util as du
import geodesic_util as gu
import netflux_util as fu
import netsolve_util as su
import network_util as nu
import pore_util as pz
import test_gpu_clearance as tc
import test_gpu_drainage as td
import test_gpu_geodesic as tg
import test_gpu_netflux as tf
import test_gpu_netsolve as ts
import test_gpu_network as tn
import test_gpu_pores as tp

# The cases the header leaves open (state `either`): (stage, when, the header's sentence). None: every case the operations below
# can reach is decided by a sentence quoted above.
EITHER = ()

STAGES = ("pores", "clearance", "network", "drainage", "geodesic", "netflux", "netsolve")
DOWNSTREAM = ("drainage", "geodesic", "netflux", "netsolve")
STEPS = ("renderScene", "dem_substep", "lbm_step")
MODULES = dict(pores=tp, clearance=tc, network=tn, drainage=td, geodesic=tg, netflux=tf, netsolve=ts)
B, T, L, R = du.SIDE_B, du.SIDE_T, du.SIDE_L, du.SIDE_R
SIDES = ((T, 4, B), (L, 3, R))
# "own": the handle's map (map == NULL); "own_copy": the same contents handed over as a caller's map; the others: callers' maps
OWN = "own"
MAPS = (OWN, "own_copy", "all_fluid", "no_fluid", "two_pores", "two_routes", "chamber_behind_neck", "chambers")
MENU = dict(pores=dict(conn=(4, 8)), clearance={}, network=dict(merge=(-1, 0, 1)), drainage=dict(sides=SIDES),
            geodesic=dict(sides=SIDES, conn=(4, 8), min_d2=(0, 4)), netflux=dict(merge=(-1, 0, 1), level=(0, 1)),
            netsolve=dict(sides=SIDES, merge=(-1, 0, 1), level=(0, 1)))
LX, LY = 48, 50          # the lattice of the single stages' callers_maps tests

Op = collections.namedtuple("Op", "kind map params")          # params: a tuple of (name, value), sorted by name


def compute(stage, map=OWN, **params):
    assert stage in STAGES and map in MAPS and sorted(params) == sorted(MENU[stage]), (stage, map, params)
    return Op(stage, map, tuple(sorted(params.items())))


def step(kind):
    assert kind in STEPS
    return Op(kind, None, ())


def show(op):
    return op.kind + ("(%s)" % ", ".join([op.map] + ["%s=%s" % kv for kv in op.params]) if op.map else "()")


def operations():
    """the full list: every stage over every map with every choice of its menu, and the three steps"""
    out = []
    for stage in STAGES:
        choices = [{}]
        for name, values in sorted(MENU[stage].items()):
            choices = [dict(c, **{name: v}) for c in choices for v in values]
        out += [compute(stage, m, **c) for m in MAPS for c in choices]
    return out + [step(k) for k in STEPS]


def callers_map(name, lx, ly, n):
    """a caller's map by name (not the two `own`s, which are the handle's to give)"""
    if name == "all_fluid":
        return np.full((lx, ly), -1, np.int32)
    if name == "no_fluid":
        return np.full((lx, ly), n, np.int32)
    if name == "chambers":          # period 4: 111 bodies and 209 links on 48 x 50 (the default 5 gives 81), one group with merge >= 0
        return su.chambers(lx, ly, period=4)
    return getattr(du, name)(lx, ly)


# ---- the walks ----

SEEDS = (0, 21, 22)
WALK_LENGTH = 40
WEIGHTS = (("pores", 2), ("clearance", 3), ("network", 4), ("drainage", 4), ("geodesic", 4), ("netflux", 4), ("netsolve", 4),
           ("renderScene", 1), ("dem_substep", 1), ("lbm_step", 1))
# the handle's map every second time, so that results are reused; among the callers' the extremes of size more often
MAP_WEIGHTS = ((OWN, 8), ("own_copy", 1), ("all_fluid", 2), ("no_fluid", 2), ("two_pores", 1), ("two_routes", 1),
               ("chamber_behind_neck", 1), ("chambers", 3))


def _pick(rng, weighted):
    """random.Random.random() alone: the one stream Python promises to keep"""
    at = rng.random() * sum(w for _, w in weighted)
    for value, w in weighted:
        at -= w
        if at < 0:
            return value
    return weighted[-1][0]


def walk(seed, length=WALK_LENGTH):
    rng = random.Random(seed)
    out = []
    for _ in range(length):
        kind = _pick(rng, WEIGHTS)
        if kind in STEPS:
            out.append(step(kind))
            continue
        m = _pick(rng, MAP_WEIGHTS)
        out.append(compute(kind, m, **{k: _pick(rng, [(v, 1) for v in vs]) for k, vs in sorted(MENU[kind].items())}))
    return out


# ---- the ordered pairs and the four stages at two merges ----

def pair_cases():
    """-> the 14 (stage, own or caller's) in order"""
    return [(s, own) for s in STAGES for own in (True, False)]


def pair_op(case, second, agree):
    """the operation of a pair's first or second member. The stages that share the network (network, netflux, netsolve; drainage
    asks for merge -1 where it runs it) agree in merge (-1) with `agree` and differ (0, then 1) without; the geodesic rides on the
    clearance (min_d2 4) with `agree`; the two members differ in everything else they can, their callers' maps included"""
    stage, own = case
    m = OWN if own else ("chambers" if second else "two_routes")
    merge = -1 if agree else (1 if second else 0)
    p = dict(pores=dict(conn=4 if second else 8), clearance={}, network=dict(merge=merge), drainage=dict(sides=SIDES[second]),
             geodesic=dict(sides=SIDES[second], conn=4 if second else 8, min_d2=4 if agree else 0),
             netflux=dict(merge=merge, level=int(second)), netsolve=dict(sides=SIDES[second], merge=merge, level=int(second)))[stage]
    return compute(stage, m, **p)


def pairs(agree):
    return [(pair_op(a, False, agree), pair_op(b, True, agree)) for a in pair_cases() for b in pair_cases()]


TWO_MERGES = (compute("netflux", merge=1, level=1), compute("netsolve", sides=SIDES[0], merge=-1, level=0),
              compute("drainage", sides=SIDES[0]), compute("network", merge=0))


# ---- the model ----

Expect = collections.namedtuple("Expect", "state result why")          # state: answers | refuses; why: what a refusal comes from


class Model:
    """per stage the (map, parameters) of its last compute and whether its readers must answer now"""

    def __init__(self):
        self.result = dict.fromkeys(STAGES)
        self.gone = dict.fromkeys(STAGES, "no compute yet")
        self.cgen = self.ngen = 0          # how many clearance and network computes have run, whoever asked
        self.cby = self.nby = None          # ... and the operation that ran the last

    def _own(self, stage):
        return self.result[stage] is not None and self.result[stage]["map"] == OWN

    def _clearance(self, m, op):
        self.cgen, self.cby = self.cgen + 1, op
        self.result["clearance"] = dict(map=m, params={}, op=op)

    def _network(self, m, merge, op):
        if not (m == OWN and self._own("clearance")):
            self._clearance(m, op)
        self.ngen, self.nby = self.ngen + 1, op
        self.result["network"] = dict(map=m, params=dict(merge=merge), op=op)

    def apply(self, op):
        if op.kind in STEPS:
            self.result = dict.fromkeys(STAGES)
            self.gone = dict.fromkeys(STAGES, op)
            return
        m, p = op.map, dict(op.params)
        mine = dict(map=m, params=p, op=op)
        if op.kind == "clearance":
            self._clearance(m, op)
            return
        if op.kind == "network":
            self._network(m, p["merge"], op)
            return
        if op.kind == "drainage":
            if not (m == OWN and self._own("network") and self._own("clearance")):
                self._network(m, -1, op)
            mine["ngen"] = self.ngen
        elif op.kind == "geodesic":
            if p["min_d2"] > 1 and not (m == OWN and self._own("clearance")):
                self._clearance(m, op)
            mine["cgen"] = self.cgen if p["min_d2"] > 1 and m == OWN else None
        elif op.kind in ("netflux", "netsolve"):
            if not (m == OWN and self._own("network") and self.result["network"]["params"]["merge"] == p["merge"]):
                self._network(m, p["merge"], op)
            mine["ngen"] = self.ngen
        self.result[op.kind] = mine

    def expect(self, stage):
        r = self.result[stage]
        if r is None:
            return Expect("refuses", None, self.gone[stage])
        if "ngen" in r and r["ngen"] != self.ngen:
            return Expect("refuses", None, self.nby)
        if r.get("cgen") is not None and r["cgen"] != self.cgen:
            return Expect("refuses", None, self.cby)
        return Expect("answers", r, None)


def trace(ops):
    """the model alone over a list of operations -> per operation {stage: Expect}"""
    model, out = Model(), []
    for op in ops:
        model.apply(op)
        out.append({s: model.expect(s) for s in STAGES})
    return out


# ---- the restatements, cached by what they are made of ----

_cache = {}


def _digest(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def restatement(stage, M, f, n, params, mkey=None, fkey=None):
    """the stage's own restatement of the map M (and the populations f, where the stage reads them). mkey, fkey: names that stand
    for the contents (a caller's map by name); otherwise their digests"""
    mkey = mkey or _digest(M)
    p = dict(params)
    net = lambda merge: _cached((mkey, n, "network", merge), lambda: nu.restate(M, n, merge))
    if stage == "clearance":
        return _cached((mkey, n, stage), lambda: cz.restate(M, n))
    if stage == "network":
        return net(p["merge"])
    if stage == "drainage":
        return _cached((mkey, n, stage, p["sides"]), lambda: du.restate(M, n, *p["sides"], N=net(-1)))
    if stage == "geodesic":
        return _cached((mkey, n, stage, p["sides"], p["conn"], p["min_d2"]), lambda: gu.restate(M, n, *p["sides"], p["conn"], p["min_d2"]))
    if stage == "netsolve":
        return _cached((mkey, n, stage, p["sides"], p["merge"], p["level"]),
                       lambda: su.restate(M, n, *p["sides"], p["merge"], p["level"], N=net(p["merge"])))
    fkey = fkey or _digest(f)
    if stage == "pores":
        return _cached((mkey, fkey, n, stage, p["conn"]), lambda: pz.restate(M, f, n, p["conn"]))
    assert stage == "netflux"
    return _cached((mkey, fkey, n, stage, p["merge"], p["level"]), lambda: fu.restate(M, f, n, p["merge"], p["level"], N=net(p["merge"])))


# ---- a handle held to the model ----

def downloading(sim, stage):
    """the stage's readers that download, by name: no device view outlives a check here"""
    mod = MODULES[stage]
    return [(who, call) for who, call in zip(mod.READERS, mod.readers_of(sim)) if not who.endswith("_device")]


def compare(sim, stage, W, counts):
    """every output the stage's downloading readers give against the restatement W, as the stage's own test compares them; counts:
    what the compute returned (a reader check passes the restatement's on)"""
    if stage == "pores":
        assert counts == W["counts"], (counts, W["counts"])
        label, table, g = sim.pore_labels(), sim.pore_table(), sim.pore_grains()
        assert label.dtype == np.int32 and np.array_equal(label, W["label"]), np.argwhere(label != W["label"])[:5]
        assert table.dtype == pz.PORE_DTYPE and len(table) == len(W["table"]), (len(table), len(W["table"]))
        for name in pz.PORE_DTYPE.names:
            assert np.array_equal(table[name], W["table"][name]), name
        for name in tp.GRAINS:
            assert g[name].dtype == np.int32 and np.array_equal(g[name], W[name]), name
    elif stage == "clearance":
        tc.compare(sim, W, counts, stage)
    elif stage == "netsolve":
        D = ts.device(sim, counts)
        assert D["counts"] == W["counts"], (D["counts"], W["counts"])
        assert su.same(D, W) is None, (su.same(D, W), D["sums"], W["sums"])
        if W["counts"]["regions"]:          # whole batches of 16 iterations, two launches each (test_gpu_netsolve.check)
            assert sim.netsolve_rounds() == 32 * max(1, -(-(W["counts"]["iterations"] + 1) // 16)), sim.netsolve_rounds()
    else:
        D = MODULES[stage].device(sim, counts)
        same = dict(network=nu, drainage=du, geodesic=gu, netflux=fu)[stage].same
        assert D["counts"] == W["counts"], (D["counts"], W["counts"])
        assert same(D, W) is None, same(D, W)
        if stage == "drainage":
            assert sim.drainage_rounds() >= (1 if len(W["passes"]) else 0)
        if stage == "geodesic":
            fwd, bwd = sim.geodesic_rounds()
            assert (fwd >= 1) == (W["counts"]["inlet_nodes"] > 0) and (bwd >= 1) == (W["counts"]["outlet_nodes"] > 0), (fwd, bwd)


def aligned(sim, stage, W, params):
    """a stage that answers is aligned with the network tables the handle shows now: the same count of links and every lo and hi"""
    if stage == "drainage":
        N, level = W["network"], 0
        assert len(sim.drainage_bodies()) == len(sim.network_bodies()) == len(N["bodies"])
        rows, table = sim.drainage_links(), N["links0"]
    else:
        level = params["level"]
        rows, table = (sim.netflux_links() if stage == "netflux" else sim.netsolve_links()), W["table"]
        assert len(sim.netflux_regions() if stage == "netflux" else sim.netsolve_regions()) == len(
            sim.network_groups() if level else sim.network_bodies())
    shown = sim.network_links(level)
    assert len(rows) == len(shown) == len(table), (len(rows), len(shown), len(table))
    for name in ("lo", "hi", "edges", "saddle"):
        assert np.array_equal(shown[name], table[name]), name


class Harness:
    """one handle (and, for the walks, a twin that takes the steps alone), the model next to it, the operations so far"""

    def __init__(self, pkg, sim, twin=None, tag=""):
        self.pkg, self.sim, self.twin, self.tag = pkg, sim, twin, tag
        self.model, self.done = Model(), []
        self.held = {}          # per stage what its last compute was made over: M, f, the counts it returned
        self._obst = self._f = None

    # the handle's state, downloaded once per step
    def obst(self):
        if self._obst is None:
            self._obst = self.sim.obst
        return self._obst

    def f(self):
        if self._f is None:
            self._f = self.sim.f
        return self._f

    def where(self):
        return "%s operation %d of %s" % (self.tag, len(self.done) - 1, [show(o) for o in self.done])

    def run(self, op):
        """the operation on the handle and on the model; a compute's own return against its restatement"""
        sim = self.sim
        self.done.append(op)
        self.model.apply(op)
        if op.kind in STEPS:
            for s in (sim, self.twin):
                if s is not None:
                    s.renderScene(s.cfg.npDEM + 1) if op.kind == "renderScene" else getattr(s, op.kind)()
            self._obst = self._f = None
            self.held = {}
            return
        p = dict(op.params)
        own = op.map in (OWN, "own_copy")
        M = self.obst() if own else callers_map(op.map, sim.lx, sim.ly, sim.n)
        arg = None if op.map == OWN else M
        try:
            if op.kind == "pores":
                got = sim.pores(p["conn"], arg)
            elif op.kind == "clearance":
                got = sim.clearance(arg)
            elif op.kind == "network":
                got = sim.network(arg, p["merge"])
            elif op.kind == "drainage":
                got = sim.drainage(*p["sides"], arg)
            elif op.kind == "geodesic":
                got = sim.geodesic(*p["sides"], p["conn"], p["min_d2"], arg)
            elif op.kind == "netflux":
                got = sim.netflux(p["merge"], p["level"], arg)
            else:
                got = sim.netsolve(*p["sides"], p["merge"], p["level"], map=arg)
        except self.pkg.LbmDemError as e:
            raise AssertionError("%s: the compute was refused: %s" % (self.where(), e))
        uses_f = op.kind in ("pores", "netflux")
        self.held[op.kind] = dict(M=M, f=self.f() if uses_f else None, mkey=None if own else op.map, counts=got)
        # the upstream stages a compute may have run are held over the same map
        for up in ("clearance", "network"):
            r = self.model.result[up]
            if r is not None and r["op"] is op and up != op.kind:
                self.held[up] = dict(M=M, f=None, mkey=None if own else op.map, counts=None)
        self.check(op.kind, counts=got)

    def check(self, stage, counts=None):
        """the stage's downloading readers against the model: a refusal with the stage's sentence, or the restatement"""
        sim, want = self.sim, self.model.expect(stage)
        if want.state == "refuses":
            for who, call in downloading(sim, stage):
                try:
                    call()
                except self.pkg.LbmDemError as e:
                    text = sim._L.lbmdem_last_error().decode()
                    assert e.code == -1 and text == MODULES[stage].NO_COMPUTE % who, (self.where(), stage, who, text)
                else:
                    raise AssertionError("%s: %s answers where the model refuses (%s)" % (self.where(), who, want.why))
            return
        held, r = self.held[stage], want.result
        W = restatement(stage, held["M"], held["f"], sim.n, r["params"], mkey=held["mkey"])
        try:
            compare(sim, stage, W, counts if counts is not None else (
                (W["counts"], W["sums"]) if stage == "netsolve" else W["counts"]))
            if stage in ("drainage", "netflux", "netsolve"):
                aligned(sim, stage, W, r["params"])
        except self.pkg.LbmDemError as e:
            raise AssertionError("%s: %s refuses where the model answers with %s: %s" % (self.where(), stage, show(r["op"]), e))
        except AssertionError as e:
            raise AssertionError("%s: %s does not answer with %s: %s" % (self.where(), stage, show(r["op"]), e))

    def check_all(self):
        for stage in STAGES:
            self.check(stage)

    def undisturbed(self):
        """what a step reads is what the twin, which made the same steps and no analysis, holds"""
        for what in ("f", "obst", "kinematics", "fhf"):
            assert np.array_equal(getattr(self.sim, what), getattr(self.twin, what)), (self.where(), what)
