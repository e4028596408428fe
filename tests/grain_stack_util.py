"""The grain-side analyses as ONE chain (include/lbmdem_hip.h, "The contact network export" through "Voronoi cells", with the coarse
and the flow fields between them): an operation list, a model of which readers must answer after any sequence of operations and with
what, and the harness that holds a handle to it. tests/test_grain_stack_host.py pins the model, tests/test_gpu_grain_stack.py the
device.

The stages share state: the clusters are made of the contact stage's records (in that stage's buffer), the Voronoi cells of the
structure stage's neighbour list and rcut, and the composite writers run computes of their own. The model below is written from the
header's sentences, not from the guards in the .hip files; the restatements it points to are the single stages' own (tests/*_util.py).

What the model encodes, each line with the sentence it comes from:
  contacts    "those of the LAST sub-step, when it was a table sub-step"; "any other sub-step or run of sub-steps,
              lbmdem_verlet_rebuild, lbmdem_upload_kinematics ... end that" (the sentence of a handle without a table sub-step); "a
              wall that lbmdem_move_walls gives another value invalidates the records" (the sentence of a moved wall) "until the next
              table sub-step"; a move that changes no wall's bits changes nothing.
  clusters    "under that call's validity condition"; the readers "are refused ... when no compute has been made for the last table
              sub-step"; "what invalidates the contact records invalidates the clusters made of them"; "a compute that is refused
              for fmin or zmin changes nothing: an earlier result stays readable"; "no call of the contact export changes a cluster
              result".
  structure   the readers "are refused ... until a compute has been made, and again after anything that moves grains: a sub-step
              (every kind of step makes some), lbmdem_upload_kinematics"; "after a compute with max_entries == 0 every reader but
              the histogram's refuses"; "a later compute replaces the result whole"; lbmdem_write_voronoi makes
              "lbmdem_structure_compute(rcut, 1, 1.0, 2^31 - 1)": "afterwards the structure readers describe that compute".
  Voronoi     "offsets, nbr and rcut of the most recent lbmdem_structure_compute, which must still be valid and must have made a
              list"; the readers are refused "exactly as the structure readers are", and after "a wall that changes value afterwards
              without a sub-step (lbmdem_move_walls, lbmdem_verlet_rebuild)"; "the cells are the Voronoi stage's own: a later
              lbmdem_structure_compute ... leaves the readers answering with the cells of the list and the rcut they were made
              with"; "a refused lbmdem_voronoi_compute discards an earlier result".
  everything  "a fluid step alone (lbmdem_lbm_step), lbmdem_upload_f, the coarse-grained and the flow fields move no grain and no
              wall: the four stages' readers go on answering".
The rebuild's VerletWall "resets Mdx, discarding its offset": on a handle whose walls have moved since the last rebuild a rebuild by
hand changes a wall's value, on any other it does not (dtt = 1 s keeps the right and the top wall at the lattice's edge)."""
import collections
import ctypes
import hashlib
import os
import random

import numpy as np

import cluster_util as cl
import coarse_util as co
import contacts_util as cu
import flow_util as fu
import structure_util as su
import test_gpu_structure as ts
import test_gpu_voronoi as tv
import voronoi_util as vu
from test_gpu_clusters import shape_packing

# The cases the header leaves open: (stage, reader), for which Model.expect says "either" and the harness takes both. None: every case the operations below can reach is decided by a sentence quoted
# above (three of them new with this harness: the refused cluster compute, the refused Voronoi compute, the fluid step alone).
EITHER = ()

# ---- the sentences of the refusals, from the single stages' tests ----
NO_TABLE = "%s: the last sub-step was no table sub-step"          # (test_gpu_contacts, test_gpu_clusters: the sentence goes on)
WALL_MOVED = "%s: a wall has been moved since the last table sub-step (lbmdem_move_walls)"          # (test_gpu_moving_walls; goes on)
NO_CLUSTERS = "%s: no lbmdem_cluster_compute has been made for the last table sub-step"          # (test_gpu_clusters.test_validity)
BAD_FMIN = "lbmdem_cluster_compute: fmin must be finite and >= 0"          # (goes on with the value)
NO_STRUCTURE, COUNTS_ONLY = ts.NO_COMPUTE, ts.COUNTS_ONLY
NO_VORONOI, NO_LIST, VORONOI_COUNTS_ONLY = tv.NO_COMPUTE, tv.NO_LIST, tv.COUNTS_ONLY
PREFIX = tuple(p.replace("%s", "") for p in (NO_TABLE, WALL_MOVED, BAD_FMIN))          # these three go on: their beginning is pinned

STAGES = ("contacts", "clusters", "structure", "voronoi")
READERS = dict(contacts=("lbmdem_contact_stats", "lbmdem_download_contacts"),
               clusters=("lbmdem_download_cluster_grains", "lbmdem_download_clusters", "lbmdem_cluster_rounds"),
               structure=("lbmdem_download_structure_grains", "lbmdem_download_structure_hist", "lbmdem_download_structure_neighbours"),
               voronoi=("lbmdem_download_voronoi_grains", "lbmdem_download_voronoi_faces"))
ALL_READERS = tuple((s, who) for s in STAGES for who in READERS[s])

# ---- the scene ----
AMP = 2.0e-6          # a shaking handle's lbmdem_move_walls moves both side walls by AMP * sin(k): half a typical overlap


def scene():
    """shape_packing(65) of the single stages' files (256 x 200; 65 grains: one more than a DEM tile; every third grain of the bottom
    row 2 um into the floor) with the last grain of the bottom row 2 um into the right wall at the lattice's edge and the first grain
    of the second row 2 um into the left wall. tests/test_grain_stack_host.py shows that it meets every inequality the comparisons
    need, so no other packing is used -> lx, ly, r, k (n x 9 kinematics)"""
    lx, ly, r, x, y, k = shape_packing(65)
    rows = np.round((y - y.min()) / 1.82e-3).astype(int)
    right = int(np.nonzero(rows == 0)[0][np.argmax(x[rows == 0])])
    left = int(np.nonzero(rows == 1)[0][np.argmin(x[rows == 1])])
    k = k.copy()
    k[right, 0] = 1e-3 * lx / 10 - r[right] + 2e-6
    k[left, 0] = r[left] - 2e-6
    k[[left, right], 3:9] = 0.0
    return lx, ly, r, k


def physics(pkg, lx, ly, r, shaking=True):
    """freq * dt = 1 rad: sin(k) is never 0, every lbmdem_move_walls of a shaking handle gives both side walls another value; a still
    handle (amp = 0) advances its clock alone. dtt = 1 s keeps the right and the top wall at the lattice's edge"""
    import vib_util
    return vib_util.physics(pkg, freq=1.0 / pkg.derive(lx, ly, r).dt, amp=AMP if shaking else 0.0)


def moved(k, times=1):
    """the kinematics of upload_moved: the topmost grain 0.6 mm higher (out of some neighbourhoods and into others), every centre
    0.2 um to the left, not at all, or to the right (other overlaps, other cells)"""
    k = np.array(k, np.float64)
    for _ in range(times):
        k[int(np.argmax(k[:, 1])), 1] += 0.6e-3
        k[:, 0] += 2e-7 * (np.arange(len(k)) % 3 - 1)
    return k


def mean_diameter(r):
    return 2.0 * float(np.mean(r))


# ---- the operations ----
Op = collections.namedtuple("Op", "kind params")          # params: a tuple of (name, value), sorted by name
CLUSTER_PARAMS = ((1.0, True, 2), (0.0, False, 1))          # (fmin, relative, zmin): test_gpu_clusters' first and last
STRUCTURE_PARAMS = ((1.1, 7, 1.2, True), (3.3, 16, 1.0, True), (2.0, 5, 1.2, False))   # (rcut / D, nbins, shell, list?)
WRITE_CLUSTERS, WRITE_STRUCTURE, WRITE_VORONOI = (0.5, True, 1), (2.5, 9, 1.1), 2.2
COARSE = ((16, 16), (8, 5))
ROOMS = ("enough", "short", "zero")
STEPS = ("dem_substep", "table_substep", "lbm_step", "renderScene", "rebuild", "upload_same", "upload_moved", "move_walls_same",
         "move_walls_other", "upload_f")
MOVES_GRAINS = ("dem_substep", "table_substep", "renderScene", "upload_same", "upload_moved")
COMPUTES = ("clusters", "structure", "voronoi", "write_clusters", "write_structure", "write_voronoi", "download_contacts",
            "write_contacts", "coarse", "flow", "grain_table")
NPDEM_PLUS_1, UPDATE_VERLET = 13, 100          # (npDEM = 12 on this lattice, asserted by the harness; the reference's updateVerlet)


def op(kind, **params):
    assert kind in STEPS + COMPUTES, kind
    return Op(kind, tuple(sorted(params.items())))


def show(o):
    return "%s(%s)" % (o.kind, ", ".join("%s=%s" % kv for kv in o.params))


def operations(shaking=None):
    """the full list; shaking True / False: the operations a shaking / a still handle can make (its lbmdem_move_walls gives the
    walls another value / the same value)"""
    out = [op("clusters", p=p) for p in CLUSTER_PARAMS] + [op("clusters", p=(-1.0, True, 2))]
    out += [op("structure", p=p) for p in STRUCTURE_PARAMS] + [op("voronoi")]
    out += [op("write_clusters", p=WRITE_CLUSTERS), op("write_structure", p=WRITE_STRUCTURE), op("write_voronoi", rcut=WRITE_VORONOI)]
    out += [op("download_contacts", room=room) for room in ROOMS] + [op("write_contacts")]
    out += [op("coarse", cell=c) for c in COARSE] + [op("flow"), op("grain_table")]
    out += [op(k) for k in STEPS]
    drop = {None: (), True: ("move_walls_same",), False: ("move_walls_other",)}[shaking]
    return [o for o in out if o.kind not in drop]


# ---- the prepared states of the pairs, and the four stateful computes at two parametrisations ----
RESET = Op("reset", ())          # the base kinematics, step counter 1, a list rebuild, a table sub-step: contacts at three walls
STATES = dict(nothing=(), everything=(op("clusters", p=CLUSTER_PARAMS[0]), op("structure", p=STRUCTURE_PARAMS[0]), op("voronoi")),
              structure_and_contacts=(op("structure", p=STRUCTURE_PARAMS[0]), op("download_contacts", room="enough")))


def pairs(shaking):
    ops = operations(shaking)
    return [(a, b) for a in ops for b in ops]


TWO_EACH = {"contacts": (op("download_contacts", room="enough"), op("write_contacts")),
            "clusters": tuple(op("clusters", p=p) for p in CLUSTER_PARAMS),
            "structure": tuple(op("structure", p=p) for p in STRUCTURE_PARAMS[:2]),
            "voronoi": (op("voronoi"), op("write_voronoi", rcut=WRITE_VORONOI))}

# ---- the walks ----
SEEDS = (58, 338, 2)          # chosen on the model alone (tests/test_grain_stack_host.py: coverage and the refusal cap)
STILL_SEED = 2          # this walk's handle has amp = 0: its lbmdem_move_walls gives the same value
WALK_LENGTH = 40
WEIGHTS = (("clusters", 9), ("structure", 6), ("voronoi", 8), ("write_clusters", 2), ("write_structure", 2), ("write_voronoi", 2),
           ("download_contacts", 4), ("write_contacts", 2), ("coarse", 3), ("flow", 2), ("grain_table", 2), ("table_substep", 3),
           ("dem_substep", 1), ("lbm_step", 2), ("renderScene", 1), ("rebuild", 1), ("upload_same", 1), ("upload_moved", 1),
           ("move_walls", 2), ("upload_f", 2))


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
    by_kind = collections.defaultdict(list)
    for o in operations():
        by_kind[o.kind].append(o)
    out = []
    for _ in range(length):
        kind = _pick(rng, WEIGHTS)
        if kind == "move_walls":
            kind = "move_walls_same" if seed == STILL_SEED else "move_walls_other"
        out.append(_pick(rng, [(o, 1) for o in by_kind[kind]]))
    return out


# ---- the model ----
Expect = collections.namedtuple("Expect", "state result sentence")          # state: answers | refuses


class Model:
    """per stage the compute its readers must answer with, or the sentence they are refused with"""

    def __init__(self, shaking):
        self.shaking = shaking
        self.kin = self.box = self.fluid = 0          # stamps of the grains', the walls' and the fluid's state (what a restatement is made over)
        self.table = None          # the stamp of the last table sub-step while the export describes it
        self.wall_moved = False          # ... and a wall has another value than that sub-step saw
        self.cl = self.st = self.vo = None
        self.nbsteps, self.mdx_off = 0, False          # the step counter; Mdx carries an offset the next rebuild discards
        self.last_table = self.uploaded = False          # the last sub-step was a table sub-step; an upload has replaced its state

    def _grains_move(self):
        self.kin += 1
        self.table, self.wall_moved = None, False
        self.cl = self.st = self.vo = None

    def _substep(self, table):
        self._grains_move()
        self.nbsteps += 1
        self.last_table, self.uploaded = table, False
        if table:
            self.table = self.kin

    def _rebuild(self):
        """-> does a wall change value"""
        self.table, self.cl = None, None
        changed, self.mdx_off = self.mdx_off, False
        if changed:
            self.box += 1
            self.vo = None
        return changed

    def _structure(self, rcut, nbins, shell, listed, by):
        self.st = dict(rcut=rcut, nbins=nbins, shell=shell, listed=listed, kin=self.kin, op=by)

    def _voronoi(self, by):
        """-> the sentence it is refused with, or None"""
        if self.st is None or not self.st["listed"]:
            self.vo = None          # "a refused lbmdem_voronoi_compute discards an earlier result"
            return NO_LIST if self.st is None else VORONOI_COUNTS_ONLY
        self.vo = dict(rcut=self.st["rcut"], kin=self.kin, box=self.box, op=by)
        return None

    def _clusters(self, p, by):
        if not (p[0] >= 0):
            return BAD_FMIN          # "changes nothing: an earlier result stays readable"
        if self.table is None or self.wall_moved:
            return (NO_TABLE if self.table is None else WALL_MOVED) % "lbmdem_cluster_compute"
        self.cl = dict(p=p, table=self.table, op=by)
        return None

    def apply(self, o):
        """-> for a compute the sentence it must be refused with (None: it must succeed); for rebuild and the moves whether a wall
        changes value"""
        k, p = o.kind, dict(o.params)
        if k == "reset":
            self._grains_move()
            self.nbsteps = 1
            self._rebuild()
            self._substep(True)
        elif k in ("dem_substep", "table_substep"):
            self._substep(k == "table_substep")
        elif k == "renderScene":
            self.fluid += 1
            for _ in range(NPDEM_PLUS_1):          # "the move, then the rebuild's reset of Mdx when nbsteps % updateVerlet == 0"
                self.mdx_off = self.mdx_off or self.shaking
                if self.nbsteps % UPDATE_VERLET == 0:
                    self.mdx_off = False
                self._substep(False)
            self.box += 1
        elif k == "rebuild":
            return self._rebuild()
        elif k in ("upload_same", "upload_moved"):
            self._grains_move()
            self.uploaded = True
        elif k == "move_walls_other":
            assert self.shaking
            self.box += 1
            self.mdx_off = True
            self.vo, self.cl = None, None
            self.wall_moved = self.table is not None
            return True
        elif k == "move_walls_same":
            assert not self.shaking
            return False
        elif k in ("clusters", "write_clusters"):
            return self._clusters(p["p"], o)
        elif k == "structure":
            self._structure(*p["p"], by=o)
        elif k == "write_structure":
            self._structure(*p["p"], listed=True, by=o)
        elif k == "voronoi":
            return self._voronoi(o)
        elif k == "write_voronoi":
            self._structure(p["rcut"], 1, 1.0, True, by=o)
            return self._voronoi(o)
        elif k in ("download_contacts", "write_contacts"):
            if self.table is None or self.wall_moved:
                return (NO_TABLE if self.table is None else WALL_MOVED) % (
                    "lbmdem_download_contacts")          # (lbmdem_write_contacts is the download, then the formatter)
        else:
            assert k in ("lbm_step", "upload_f", "coarse", "flow", "grain_table"), k
            self.fluid += k in ("lbm_step", "upload_f")
        return None

    def expect(self, stage, who):
        e = self._expect(stage, who)
        return e._replace(state="either") if (stage, who) in EITHER else e

    def _expect(self, stage, who):
        if stage == "contacts":
            if self.table is None or self.wall_moved:
                return Expect("refuses", None, (NO_TABLE if self.table is None else WALL_MOVED) % who)
            return Expect("answers", dict(table=self.table), None)
        if stage == "clusters":
            return Expect("answers", self.cl, None) if self.cl else Expect("refuses", None, NO_CLUSTERS % who)
        if stage == "structure":
            if self.st is None:
                return Expect("refuses", None, NO_STRUCTURE % who)
            if not self.st["listed"] and who != "lbmdem_download_structure_hist":
                return Expect("refuses", None, COUNTS_ONLY % who)
            return Expect("answers", self.st, None)
        assert stage == "voronoi"
        return Expect("answers", self.vo, None) if self.vo else Expect("refuses", None, NO_VORONOI % who)


def trace(ops, shaking=True, prepare=(RESET,)):
    """the model alone over a list of operations -> per operation {(stage, reader): Expect}"""
    model, out = Model(shaking), []
    for o in prepare:
        model.apply(o)
    for o in ops:
        model.apply(o)
        out.append({sw: model.expect(*sw) for sw in ALL_READERS})
    return out


# ---- the restatements, cached by what they are made of ----
_cache = {}


def _digest(*arrays):
    h = hashlib.sha1()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def structure_restatement(x, y, r, rcut, nbins, shell):
    A = _cached(("structure", _digest(x, y, r)), lambda: su.Restatement(x, y, r))
    return _cached(("structure", _digest(x, y, r), rcut, nbins, shell), lambda: A.at(rcut, nbins, shell))


def voronoi_restatement(x, y, r, box, rcut):
    A = _cached(("voronoi", _digest(x, y, r), box), lambda: vu.Restatement(x, y, r, box))
    return _cached(("voronoi", _digest(x, y, r), box, rcut), lambda: A.at(rcut))


def cluster_restatement(rec, n, x1, x2, p):
    return _cached(("clusters", _digest(rec, x1, x2), p), lambda: cl.restate(rec, n, x1, x2, *p))


def all_pairs(n):
    """every pair i < j in the reference's loop order: a list that holds every pair holds every pair that touches"""
    i, j = np.triu_indices(n, 1)
    return np.stack([i, j], axis=1)


def contact_lines(rec):
    return "# i j dn nx ny fn ft\n" + "".join("%d %d %e %e %e %e %e\n" % (c["i"], c["j"], c["dn"], c["nx"], c["ny"], c["fn"], c["ft"])
                                              for c in rec)


def same_rows(a, b):
    return a.dtype == b.dtype and len(a) == len(b) and all(a[f].tobytes() == b[f].tobytes() for f in a.dtype.names)


# ---- a handle held to the model ----
class Harness:
    """one handle (and, for the walks, a twin that makes only the steps), the model next to it, the operations so far"""

    def __init__(self, pkg, sim, r, k0, shaking, tmp, twin=None, tag=""):
        self.pkg, self.sim, self.twin, self.tag = pkg, sim, twin, tag
        self.r, self.k0, self.tmp = np.asarray(r, np.float64), np.array(k0, np.float64), str(tmp)
        self.model, self.done, self.files = Model(shaking), [], 0
        self.D = mean_diameter(r)
        self.kin = {}          # the model's stamp -> (x, y) of the grains in that state
        self.boxes = {}          # the model's stamp of the walls -> the four walls a Voronoi compute found
        self.tables = {}          # ... of a table sub-step -> its restated records, counters and the table's columns
        self.L = pkg.load_library()
        for s in self.both():
            s.set_vibration(True)
        assert sim.cfg.npDEM + 1 == NPDEM_PLUS_1 and sim.config().phys.updateVerlet == UPDATE_VERLET

    def both(self):
        return [s for s in (self.sim, self.twin) if s is not None]

    def where(self):
        return "%s operation %d of %s" % (self.tag, len(self.done) - 1, [show(o) for o in self.done])

    def box(self):
        w = self.sim.walls()
        return w["Mgx"], w["Mdx"], w["Mby"], w["Mhy"]

    def centres(self):
        if self.model.kin not in self.kin:
            k = self.sim.kinematics
            self.kin[self.model.kin] = (k[:, 0].copy(), k[:, 1].copy())
        return self.kin[self.model.kin]

    def stamps(self):
        """what the coarse and the flow fields read has not changed while these have not: their restatements are made once per
        state, so a compute in between that disturbed a population or a grain would show in the next comparison"""
        m = self.model
        return m.kin, m.box, m.fluid, m.last_table

    def text(self):
        return self.L.lbmdem_last_error().decode()

    def refused(self, call, sentence, what):
        """call() must be refused with the sentence (its beginning, where the single stages pin no more)"""
        try:
            call()
        except self.pkg.LbmDemError as e:
            text = self.text()
            whole = not sentence.endswith(PREFIX)
            assert e.code == -1 and (text == sentence if whole else text.startswith(sentence)), (self.where(), what, text, sentence)
        else:
            raise AssertionError("%s: %s answers where the model refuses with '%s'" % (self.where(), what, sentence))

    def _table_substep(self):
        """the handle's table sub-step and its restatement: tests/test_gpu_contacts.py's `restated`"""
        pre = None
        for s in self.both():
            s.set_diagnostics(True)
            if s is self.sim:
                pre, film = s.kinematics, s.nbsteps % s.config().phys.stepFilm == 0
            s.dem_substep()
        sim = self.sim
        cumul, neigh, wf = sim.verlet()
        P = cu.params_of_config(sim.config())
        rec, counts = cu.restate(pre, self.r, cu.pairs_of_list(cumul, neigh), wf, P, film)
        T = sim.grain_table()
        self.tables[self.model.table] = dict(rec=rec, counts=counts, x1=T[:, 0].copy(), x2=T[:, 1].copy(), fm=T[:, 18].copy(),
                                             radius=T[:, 9].copy())

    def run(self, o):
        """the operation on the handle (and the twin) and on the model; a compute's own return against its restatement"""
        sim, k, p = self.sim, o.kind, dict(o.params)
        self.done.append(o)
        box0 = self.box() if k in ("rebuild", "move_walls_same", "move_walls_other") else None
        want = self.model.apply(o)
        try:
            if k == "reset":
                for s in self.both():
                    s.kinematics = self.k0
                    s.nbsteps = 1
                    s.initVerlet()
                self._table_substep()
            elif k == "table_substep":
                self._table_substep()
            elif k == "dem_substep":
                for s in self.both():
                    s.set_diagnostics(False)
                    s.dem_substep()
            elif k == "renderScene":
                for s in self.both():
                    s.set_diagnostics(False)
                    s.renderScene(NPDEM_PLUS_1)
            elif k == "lbm_step":
                for s in self.both():
                    s.lbm_step()
            elif k == "upload_f":
                for s in self.both():
                    s.f = s.f
            elif k in ("rebuild", "move_walls_same", "move_walls_other"):
                for s in self.both():
                    s.initVerlet() if k == "rebuild" else s.move_walls()
                assert (self.box() != box0) == want, (self.where(), box0, self.box())
            elif k in ("upload_same", "upload_moved"):
                for s in self.both():
                    s.kinematics = s.kinematics if k == "upload_same" else moved(s.kinematics)
            else:
                self.compute(o, want)
        except self.pkg.LbmDemError as e:
            raise AssertionError("%s: refused: %s" % (self.where(), e))
        if self.model.nbsteps:
            assert sim.nbsteps == self.model.nbsteps, (self.where(), sim.nbsteps, self.model.nbsteps)

    def compute(self, o, sentence):
        sim, k, p = self.sim, o.kind, dict(o.params)
        D = self.D
        self.files += 1
        out = os.path.join(self.tmp, "%s%03d" % (k, self.files))
        if k.startswith("write_"):
            os.makedirs(out)
        call = {"clusters": lambda: sim.clusters(*p["p"]), "write_clusters": lambda: sim.write_clusters(out, 7, *p["p"]),
                "structure": lambda: sim.structure(p["p"][0] * D, p["p"][1], p["p"][2], **({} if p["p"][3] else dict(max_entries=0))),
                "write_structure": lambda: sim.write_structure(out, 7, p["p"][0] * D, *p["p"][1:]),
                "voronoi": lambda: sim.voronoi(), "write_voronoi": lambda: sim.write_voronoi(out, 7, p["rcut"] * D),
                "write_contacts": lambda: sim.write_contacts(out, 7)}.get(k)
        if sentence is not None and k != "download_contacts":
            self.refused(call, sentence, show(o))
            if k.startswith("write_"):
                assert os.listdir(out) == [], (self.where(), os.listdir(out))
            return
        x, y = self.centres()
        t = sim.nbsteps * sim.config().dt
        if k in ("clusters", "write_clusters"):
            T = self.tables[self.model.table]
            R = cluster_restatement(T["rec"], sim.n, T["x1"], T["x2"], p["p"])
            got = call()
            if k == "clusters":
                assert got[0] == R["counts"] and cl.same_bits(got[1], R["thr"]), (self.where(), got, R["counts"], R["thr"])
            else:
                files = cl.files_text(T["radius"], T["x1"], T["x2"], T["fm"], T["rec"], R, *p["p"], t, sim.lx, sim.ly)
                names = ("clusters000007.dat", "cluster_table000007.dat", "DEM000007_clusters.ps", "clusters.data")
                assert sorted(os.listdir(out)) == sorted(names), self.where()
                for name, text in zip(names, files[:3] + (cl.DATA_HEADER + files[3],)):
                    assert open(os.path.join(out, name)).read() == text, (self.where(), name)
        elif k in ("structure", "write_structure"):
            rcut, nbins, shell = p["p"][0] * D, p["p"][1], p["p"][2]
            R = structure_restatement(x, y, self.r, rcut, nbins, shell)
            got = call()
            if k == "structure":
                assert got == R["counts"], (self.where(), got, R["counts"])
            else:
                b = self.box()
                files = su.files_text(R["grains"], rcut, nbins, shell, R["hist"], R["counts"], t, b[1] - b[0], b[3] - b[2])
                names = ("structure000007.dat", "gr000007.dat", "structure.data")
                assert sorted(os.listdir(out)) == sorted(names), self.where()
                for name, text in zip(names, files[:2] + (su.DATA_HEADER + files[2],)):
                    assert open(os.path.join(out, name)).read() == text, (self.where(), name)
        elif k in ("voronoi", "write_voronoi"):
            rcut, b = self.model.vo["rcut"] * D, self.box()
            assert self.boxes.setdefault(self.model.box, b) == b, (self.where(), self.boxes[self.model.box], b)
            R = voronoi_restatement(x, y, self.r, b, rcut)
            got = call()
            if k == "voronoi":
                assert got == R["counts"], (self.where(), got, R["counts"])
            else:
                files = vu.files_text(R["grains"], rcut, R["counts"], t, b[1] - b[0], b[3] - b[2])
                assert sorted(os.listdir(out)) == ["voronoi.data", "voronoi000007.dat"], self.where()
                assert open(os.path.join(out, "voronoi000007.dat")).read() == files[0], self.where()
                assert open(os.path.join(out, "voronoi.data")).read() == vu.DATA_HEADER + files[1], self.where()
        elif k == "download_contacts":
            self.download_contacts(p["room"], sentence)
        elif k == "write_contacts":
            T = self.tables[self.model.table]
            call()
            assert sorted(os.listdir(out)) == ["DEM000007_chains.ps", "contacts000007.dat"], self.where()
            assert open(os.path.join(out, "contacts000007.dat")).read() == contact_lines(T["rec"]), self.where()
            ps = open(os.path.join(out, "DEM000007_chains.ps")).read()
            head = cl.ps_head(T["radius"], T["x1"], T["x2"], T["fm"], sim.lx, sim.ly)
            assert ps.startswith(head) and ps.count("stroke") == int(((T["rec"]["j"] >= 0) & (T["rec"]["fn"] > 0)).sum()), self.where()
        elif k == "coarse":
            cw, ch = p["cell"]
            want = _cached(("coarse", id(self), cw, ch) + self.stamps(), lambda: co.expected(sim, self.r, cw, ch))
            assert want[2] == int(self.model.last_table), (self.where(), want[2])
            cells, outside, valid = sim.coarse_fields(cw, ch)
            assert not co.mismatches(cells, want[0]) and (outside, valid) == want[1:], (self.where(), co.mismatches(cells, want[0]))
        elif k == "flow":
            F, sums = _cached(("flow", id(self)) + self.stamps(), lambda: fu.expected(sim))
            assert not fu.mismatches(sim.flow_fields(), F), self.where()
            assert sim.flow_sums() == sums, (self.where(), sim.flow_sums(), sums)
        else:
            assert k == "grain_table"
            if self.model.last_table:          # "the condition of lbmdem_download_grain_table": the last sub-step was a table sub-step
                T = sim.grain_table()
                assert cl.same_bits(T[:, 9], self.r), self.where()
                if not self.model.uploaded:
                    assert cl.same_bits(T[:, 0], x) and cl.same_bits(T[:, 1], y), self.where()

    def download_contacts(self, room, sentence):
        """lbmdem_download_contacts with room for every record, for one record fewer, for none (the count alone)"""
        sim, vp = self.sim, lambda a: a.ctypes.data_as(ctypes.c_void_p)
        cnt = ctypes.c_long(-1)
        if sentence is not None:
            buf = np.full(4, 7, cu.CONTACT_DTYPE)
            rc = self.L.lbmdem_download_contacts(sim._h, vp(buf) if room != "zero" else None, 0 if room == "zero" else 4, ctypes.byref(cnt))
            assert rc == -1 and self.text().startswith(sentence) and (buf["i"] == 7).all(), (self.where(), rc, self.text())
            return
        rec = self.tables[self.model.table]["rec"]
        assert len(rec) > 1
        if room == "zero":
            assert self.L.lbmdem_download_contacts(sim._h, None, 0, ctypes.byref(cnt)) == 0 and cnt.value == len(rec), self.where()
        elif room == "short":
            small = np.full(len(rec) - 1, 7, cu.CONTACT_DTYPE)
            assert self.L.lbmdem_download_contacts(sim._h, vp(small), len(small), ctypes.byref(cnt)) == -1, self.where()
            assert cnt.value == len(rec) and (small["i"] == 7).all() and (small["fn"] == 7).all(), self.where()
            assert self.text() == "lbmdem_download_contacts: there are %d records, the buffer holds %d" % (len(rec), len(small))
        else:
            buf = np.full(len(rec) + 3, 7, cu.CONTACT_DTYPE)
            assert self.L.lbmdem_download_contacts(sim._h, vp(buf), len(buf), ctypes.byref(cnt)) == 0 and cnt.value == len(rec)
            assert cu.same_records(buf[:len(rec)], rec) and (buf["i"][len(rec):] == 7).all(), self.where()

    # ---- the readers ----
    def calls(self, stage):
        sim = self.sim
        out = dict(contacts=(sim.contact_stats, sim.download_contacts),
                   clusters=(sim.cluster_grains, sim.cluster_table, sim.cluster_rounds),
                   structure=(sim.structure_grains, sim.structure_hist, sim.structure_neighbours),
                   voronoi=(sim.voronoi_grains, sim.voronoi_faces))[stage]
        return list(zip(READERS[stage], out))

    def check(self, stage):
        """the stage's downloading readers against the model: a refusal with the stage's sentence, or the restatement"""
        for who, call in self.calls(stage):
            e = self.model.expect(stage, who)
            if e.state == "either":          # a case of EITHER: an answer is held to the restatement, a refusal to the sentence
                try:
                    self.compare(stage, who, call(), e.result)
                except self.pkg.LbmDemError:
                    assert self.text() == e.sentence, (self.where(), who, self.text())
                continue
            if e.state == "refuses":
                self.refused(call, e.sentence, who)
                continue
            try:
                got = call()
                self.compare(stage, who, got, e.result)
            except self.pkg.LbmDemError as err:
                raise AssertionError("%s: %s refuses where the model answers: %s" % (self.where(), who, err))
            except AssertionError as err:
                by = e.result.get("op")
                raise AssertionError("%s: %s does not answer with %s: %s" % (self.where(), who, show(by) if by else "the table sub-step", err))

    def compare(self, stage, who, got, result):
        D = self.D
        if stage in ("structure", "voronoi"):          # the grains and the walls of the compute the model names, not the present ones
            x, y = self.kin[result["kin"]]
        if stage == "contacts":
            T = self.tables[result["table"]]
            if who == "lbmdem_contact_stats":
                assert got == T["counts"], (got, T["counts"])
            else:
                assert cu.same_records(got, T["rec"]), (len(got), len(T["rec"]))
        elif stage == "clusters":
            T = self.tables[result["table"]]
            R = cluster_restatement(T["rec"], self.sim.n, T["x1"], T["x2"], result["p"])
            if who == "lbmdem_download_cluster_grains":
                for name in ("label", "degree", "core", "walls"):
                    assert got[name].dtype == np.int32 and np.array_equal(got[name], R[name]), name
            elif who == "lbmdem_download_clusters":
                assert cl.same_table(got, R["table"]), (got, R["table"])
            else:
                assert got[1] == R["peel_rounds"] and 0 <= got[0] <= self.sim.n + 1, (got, R["peel_rounds"])
        elif stage == "structure":
            R = structure_restatement(x, y, self.r, result["rcut"] * D, result["nbins"], result["shell"])
            if who == "lbmdem_download_structure_grains":
                assert same_rows(got, R["grains"]), [f for f in got.dtype.names if got[f].tobytes() != R["grains"][f].tobytes()]
            elif who == "lbmdem_download_structure_hist":
                assert got.dtype == np.int64 and np.array_equal(got, R["hist"]), (len(got), len(R["hist"]))
            else:
                assert got[0].dtype == got[1].dtype == np.int32
                assert np.array_equal(got[0], R["offsets"]) and np.array_equal(got[1], R["nbr"]), (len(got[1]), len(R["nbr"]))
        else:
            R = voronoi_restatement(x, y, self.r, self.boxes[result["box"]], result["rcut"] * D)
            if who == "lbmdem_download_voronoi_grains":
                assert same_rows(got, R["grains"]), [f for f in got.dtype.names if got[f].tobytes() != R["grains"][f].tobytes()]
            else:
                off, src, length = got
                assert off.dtype == src.dtype == np.int32 and length.dtype == np.float64
                assert np.array_equal(off, R["foff"]) and np.array_equal(src, R["fsrc"]) and vu.same_bits(length, R["flen"])

    def check_all(self):
        for stage in STAGES:
            self.check(stage)

    def undisturbed(self):
        """what a step reads is what the twin, which made the same steps and no analysis, holds"""
        for what in ("f", "obst", "kinematics", "fhf"):
            assert np.array_equal(getattr(self.sim, what), getattr(self.twin, what)), (self.where(), what)
        assert self.sim.walls() == self.twin.walls(), self.where()
