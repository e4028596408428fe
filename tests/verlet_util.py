"""The reference's Verlet rebuild restated in numpy float64 (initVerlet + VerletWall, main.c:1519-1594), and generators
of grain placements that sit on the thresholds of the library's cell grid. Shared by tests/test_verlet_host.py (no GPU)
and tests/test_gpu_verlet_edges.py.

all_pairs and wall_flags form EXPECTED values: plain all-pairs loops in the reference's association, nothing of the grid.
grid_cells, grid_shape and cell_edge restate the library (cell_coord, verlet_alloc, lbmdem_create) and are used only to
AIM inputs at cell boundaries and to count how many accepted pairs a 3 x 3 cell scan could not see."""
import numpy as np

DV = 5e-4                  # distVerlet of lbmdem_physics_defaults
CELL_PAD = 1.001           # the library's cell edge: (2 rmax + distVerlet) * CELL_PAD (lbmdem_create)
ORIGINS = ((0.0, 0.0), (3.3e-4, 1e-4))   # the reference's Mgx, Mby; walls elsewhere (a config of the caller's, a restart)
# the placement the CPU search for the unpadded cell edge found first: accepted by the reference's test at
# origin 3.3e-4, cells 2 and 4 of a grid with edge 2 rmax + distVerlet
STRADDLER = dict(rmax=float.fromhex("0x1.d9878fc873ab0p-12"), ox=0.00033,
                 xi=float.fromhex("0x1.29812411ffe04p-8"), xj=float.fromhex("0x1.8576b1b0f1a99p-8"))


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def pair_lhs(rl, xl, yl, rh, xh, yh):
    """the three left-hand sides of main.c:1529-1532 for lo < hi (one rounding per operation)"""
    ddx, ddy = xl - xh, yl - yh
    return np.abs(ddx) - rl - rh, np.abs(ddy) - rl - rh, np.sqrt(ddx * ddx + ddy * ddy) - rl - rh


def pair_accepted(rl, xl, yl, rh, xh, yh, dV=DV):
    a, b, c = pair_lhs(rl, xl, yl, rh, xh, yh)
    return (a <= dV) & (b <= dV) & (c <= dV)


def all_pairs(r, x1, x2, dV=DV):
    """initVerlet (main.c:1519-1541) over all pairs -> (cumul[n], neighbours[npairs]): for every i its partners j > i,
    ascending; cumul[i] the running end offset, never written for the last grain (it stays the 0 of the memset)."""
    r, x1, x2 = _f(r), _f(x1), _f(x2)
    n = len(r)
    hit = pair_accepted(r[:, None], x1[:, None], x2[:, None], r[None, :], x1[None, :], x2[None, :], dV)
    hit &= np.arange(n)[None, :] > np.arange(n)[:, None]
    cumul = np.cumsum(hit.sum(1)).astype(np.int32)
    cumul[-1] = 0
    return cumul, np.nonzero(hit)[1].astype(np.int32)


def wall_flags(r, x1, x2, Mby, Mhy, Mgx, Mdx, dV=DV):
    """VerletWall's four candidate lists (main.c:1563-1593) as flags: bit 0 bottom, 1 top, 2 left, 3 right"""
    r, x1, x2 = _f(r), _f(x1), _f(x2)
    f = np.zeros(len(r), np.int32)
    f |= np.where(x2 - r - Mby < dV, 1, 0).astype(np.int32)
    f |= np.where(-x2 - r + Mhy < dV, 2, 0).astype(np.int32)
    f |= np.where(x1 - r - Mgx < dV, 4, 0).astype(np.int32)
    f |= np.where(-x1 - r + Mdx < dV, 8, 0).astype(np.int32)
    return f


def wall_lhs(r, x1, x2, Mby, Mhy, Mgx, Mdx):
    """the four left-hand sides of those tests, [4][n]"""
    r, x1, x2 = _f(r), _f(x1), _f(x2)
    return np.stack([x2 - r - Mby, -x2 - r + Mhy, x1 - r - Mgx, -x1 - r + Mdx])


# ---- the library's grid: for aiming only -------------------------------------------------------------------------------
def cell_edge(rmax, dV=DV, pad=CELL_PAD):
    return (2 * rmax + dV) * pad


def grid_shape(lx, ly, dx, cs):
    """ncx, ncy of verlet_alloc over a lattice of lx x ly nodes"""
    return int(np.ceil(dx * (lx - 1) / cs)) + 1, int(np.ceil(dx * (ly - 1) / cs)) + 1


def grid_cells(x, o, cs, nc):
    """cell_coord of dem_kernels.hip: floor((x - o) / cs) clamped into 0 .. nc - 1"""
    return np.clip(np.floor((_f(x) - o) / cs), 0, nc - 1).astype(np.int64)


def lattice_dx(lx):
    """dx of lbmdem_derive at scale 1 (main.c:1837, 1844)"""
    return (1. / 1.0) * (1.e-3 * lx / 10 - 0.) / (lx - 1)


def ulps(x, m):
    """the double m steps above (below: m < 0) a positive finite x"""
    return (np.asarray(x, dtype=np.float64).view(np.int64) + np.int64(m)).view(np.float64)


def first_of_cell(k, o, cs, nc):
    """the smallest double whose cell is k (1 <= k <= nc - 1); the double below it is the last of cell k - 1"""
    assert 1 <= k <= nc - 1
    x = np.float64(o + k * cs)
    while grid_cells(x, o, cs, nc) >= k:
        x = np.nextafter(x, -np.inf)
    while grid_cells(x, o, cs, nc) < k:
        x = np.nextafter(x, np.inf)
    return float(x)


PAIR_DTYPE = np.dtype([("ri", "f8"), ("rj", "f8"), ("xi", "f8"), ("yi", "f8"), ("xj", "f8"), ("yj", "f8"),
                       ("axis", "U1"), ("place", "U5"), ("m", "i4")])


def _aim(place, k, o, cs, nc):
    if place == "last":
        return float(np.nextafter(first_of_cell(k, o, cs, nc), -np.inf))
    if place == "first":
        return first_of_cell(k, o, cs, nc)
    return o + (k - 0.5) * cs


def threshold_pairs(rng, rmax, rsmall, lx, ly, origin=(0.0, 0.0), dV=DV, axes="xyd", pads=(1.0, CELL_PAD), span=3):
    """Pairs (i, j) on the candidate test's threshold and on the grid's cell boundaries, as records of PAIR_DTYPE.

    x (y) pairs: xi is the last double of cell k - 1, the first of cell k, or mid-cell, the boundary taken from the grid with
    edge (2 rmax + dV) * pad for every pad asked for; xj = xi +- (ri + rj + dV) moved by -span .. +span ulps, so the sweep
    holds pairs the reference accepts, pairs it rejects by an ulp and (most sweeps) one exactly on equality; for radii (rmax,
    rmax) that distance is the unpadded cell edge. The other coordinate is free (NaN): pack() chooses it, the same for both.
    d pairs: both coordinates of i aimed like that, j at the threshold distance in a direction drawn from rng, where both
    fabs tests pass and the sqrt decides; plus, where a search of +-8 ulps in both coordinates finds one, a placement with
    the sqrt's left-hand side exactly distVerlet (m = 99). The boundary k: the last (nc - 1) and the first in turn, then any."""
    ox, oy = origin
    dx = lattice_dx(lx)
    out = []
    count = [0]
    side = 1.0

    def boundary(nc, sgn):
        """the last boundary, the first, then any (a j below i needs a cell below i's for it)"""
        count[0] += 1
        lo = 2 if sgn < 0 else 1
        return (nc - 1, lo)[count[0] % 2] if count[0] <= 12 else int(rng.integers(lo, nc))

    for pad in pads:
        cs = cell_edge(rmax, dV, pad)
        ncx, ncy = grid_shape(lx, ly, dx, cs)
        for axis in axes:
            for place in ("last", "first", "mid"):
                if place == "mid" and pad != pads[0]:
                    continue
                for (ri, rj) in ((rmax, rmax), (rmax, rsmall), (rsmall, rmax)):
                    if ri != rj and pad != pads[0]:
                        continue
                    for sgn in ((1.0, -1.0) if ri == rj and axis != "d" else (side,)):   # j above i, below i
                        side = -side
                        reach = ri + rj + dV
                        if axis == "x":
                            xi = _aim(place, boundary(ncx, sgn), ox, cs, ncx)
                            for m in range(-span, span + 1):
                                out.append((ri, rj, xi, np.nan, float(ulps(xi + sgn * reach, m)), np.nan, axis, place, m))
                        elif axis == "y":
                            yi = _aim(place, boundary(ncy, sgn), oy, cs, ncy)
                            for m in range(-span, span + 1):
                                out.append((ri, rj, np.nan, yi, np.nan, float(ulps(yi + sgn * reach, m)), axis, place, m))
                        else:
                            th = rng.uniform(0.3, 1.27)
                            for m in range(-span, span + 2):
                                xi, yi = _aim(place, boundary(ncx, sgn), ox, cs, ncx), _aim(place, boundary(ncy, -1), oy, cs, ncy)
                                xj0, yj0 = xi + sgn * reach * np.cos(th), yi - reach * np.sin(th)
                                if m <= span:
                                    out.append((ri, rj, xi, yi, float(ulps(xj0, m)), yj0, axis, place, m))
                                    continue
                                mm = np.arange(-8, 9)
                                xs, ys = np.meshgrid(ulps(xj0, mm), ulps(yj0, mm), indexing="ij")
                                eq = np.argwhere(pair_lhs(ri, xi, yi, rj, xs, ys)[2] == dV)
                                if len(eq):
                                    out.append((ri, rj, xi, yi, float(xs[tuple(eq[0])]), float(ys[tuple(eq[0])]), axis, place, 99))
    return np.array(out, dtype=PAIR_DTYPE)


def pack(pairs, rmax, lx, ly, origin=(0.0, 0.0), dV=DV, max_grains=300, seed=5):
    """Distribute threshold pairs over as few scenes (one handle each) as it takes: every grain farther than the widest
    candidate distance from every grain of another pair, on one axis at least, so a pair's partner is the only grain its
    members can be listed with; a free coordinate gets a value inside the lattice. -> [(r, x1, x2)], i = 2 p, j = 2 p + 1.
    Every scene holds a grain of radius rmax (each pair does), so its cell edge is the one the pairs were aimed at."""
    rng = np.random.default_rng(seed)
    ox, oy = origin
    W, H = lattice_dx(lx) * (lx - 1), lattice_dx(lx) * (ly - 1)
    clear = 1.05 * (2 * rmax + dV)
    scenes = []   # lists of (r, x, y)
    for p in pairs:
        placed = False
        for sc in scenes + [None]:
            if sc is None:
                sc = []
                scenes.append(sc)
            if len(sc) + 2 > max_grains:
                continue
            g = np.array([(x, y) for (_, x, y) in sc]).reshape(-1, 2)
            for _ in range(120):
                xi, yi, xj, yj = p["xi"], p["yi"], p["xj"], p["yj"]
                if np.isnan(xi):
                    xi = xj = ox + rng.uniform(0.03, 0.97) * W
                if np.isnan(yi):
                    yi = yj = oy + rng.uniform(0.03, 0.97) * H
                new = np.array([(xi, yi), (xj, yj)])
                if len(g) == 0 or (np.abs(g[:, None, :] - new[None, :, :]).max(2) > clear).all():
                    sc.append((p["ri"], xi, yi)); sc.append((p["rj"], xj, yj))
                    placed = True
                    break
                if not (np.isnan(p["xi"]) or np.isnan(p["yi"])):
                    break   # nothing free to draw again
            if placed:
                break
        assert placed
    return [tuple(np.array(c) for c in zip(*sc)) for sc in scenes]


def straddlers(r, x1, x2, origin, cs, lx, ly, dV=DV):
    """(accepted pairs, those whose cells -- of a grid with edge cs -- are more than one apart on an axis: a 3 x 3 scan
    never tests them)"""
    r, x1, x2 = _f(r), _f(x1), _f(x2)
    ncx, ncy = grid_shape(lx, ly, lattice_dx(lx), cs)
    cumul, nb = all_pairs(r, x1, x2, dV)
    cnt = np.diff(np.concatenate([[0], cumul[:-1], [len(nb)]]))
    i = np.repeat(np.arange(len(r)), cnt)
    cx, cy = grid_cells(x1, origin[0], cs, ncx), grid_cells(x2, origin[1], cs, ncy)
    far = (np.abs(cx[i] - cx[nb]) > 1) | (np.abs(cy[i] - cy[nb]) > 1)
    return len(nb), int(far.sum())


def search_straddlers(rng, n, origin, pad, dV=DV, kmax=400):
    """n random placements on the threshold, vectorised: rmax from 0.05 .. 1.5 mm; the partner's radius rmax (half of them)
    or 0.5 .. 1 of it, in either order; i at the last double of cell k - 1 or the first of cell k (k = 1 .. kmax) of the grid
    with edge (2 rmax + dV) * pad on both axes, or anywhere in the cell; j at the threshold distance ri + rj + dV along x,
    along y, or in a direction theta -- a quarter of them within 1e-9 .. 1e-3 rad of an axis, where the sqrt passes while one
    coordinate's distance is still the whole edge -- moved by -1 .. +3 ulps, on either side. -> (placements the reference
    accepts, those of them more than one cell apart on an axis)"""
    ox, oy = origin
    rmax = rng.uniform(0.05e-3, 1.5e-3, n)
    rs = np.where(rng.random(n) < 0.5, rmax, rmax * rng.uniform(0.5, 1.0, n))
    swap = rng.random(n) < 0.5
    ri, rj = np.where(swap, rs, rmax), np.where(swap, rmax, rs)
    cs = (2 * rmax + dV) * pad
    nc = kmax + 2

    def aimed(o):
        k = rng.integers(1, kmax + 1, n)
        x = o + k * cs
        cand = np.stack([ulps(x, m) for m in range(-4, 5)])                # ascending
        first = cand[np.argmax(grid_cells(cand, o, cs, nc) >= k, axis=0), np.arange(n)]
        how = rng.integers(0, 3, n)
        return np.where(how == 0, ulps(first, -1), np.where(how == 1, first, o + (k - rng.random(n)) * cs))

    xi, yi = aimed(ox), aimed(oy)
    kind = rng.integers(0, 4, n)
    th = np.where(kind == 0, 0.0, np.where(kind == 1, np.pi / 2, np.where(kind == 2, 10.0 ** rng.uniform(-9, -3, n),
                                                                     rng.uniform(0.0, np.pi / 2, n))))
    th = np.where((kind == 2) & (rng.random(n) < 0.5), np.pi / 2 - th, th)
    reach = ri + rj + dV
    sx, sy = rng.choice([-1.0, 1.0], n), rng.choice([-1.0, 1.0], n)
    cx_, sn_ = np.where(kind == 1, 0.0, np.cos(th)), np.where(kind == 0, 0.0, np.sin(th))
    m = rng.integers(-1, 4, n)
    xj = np.where(kind == 1, xi, ulps(np.abs(xi + sx * reach * cx_) + 1e-300, m))
    yj = np.where(kind == 0, yi, ulps(np.abs(yi + sy * reach * sn_) + 1e-300, m))
    ok = pair_accepted(ri, xi, yi, rj, xj, yj, dV)
    far = (np.abs(grid_cells(xi, ox, cs, nc) - grid_cells(xj, ox, cs, nc)) > 1) | \
          (np.abs(grid_cells(yi, oy, cs, nc) - grid_cells(yj, oy, cs, nc)) > 1)
    return int(ok.sum()), int((ok & far).sum())
