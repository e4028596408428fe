"""Two-dimensional synthetic packings for the tests (inputs only; samples.row_packing lays rows that never touch each other).

tri_packing: a triangular lattice of pitch 2 rmean -- odd rows shifted by half a pitch, rows pitch sqrt(3) / 2 apart -- with
radii rmean + U(-spread, spread) and centres jittered by N(0, noise) in both directions. With spread and noise of a few
microns about half of a grain's six lattice neighbours touch it: most grains carry three or more non-zero contact forces
(their sum depends on the order of the additions), two thirds of the contact normals are 60 degrees from horizontal, and at
reductionR >= 1 a reduced disc meets six others.

census / check_scene: the conditions the tests put on such a scene, from the geometry alone (numpy). Units: millimetres, as
in samples.py; 0.1 mm per lattice node."""
import numpy as np

import samples

SQ3_2 = np.sqrt(3.0) / 2.0
# what a scene of the packed tests has to be (tests/test_packing_host.py, and again at the top of every GPU test)
MIN_FRAC_3_PARTNERS = 0.40      # grains with three or more touching partners
MIN_FRAC_STEEP = 0.50           # touching pairs whose normal is steeper than 45 degrees
MAX_OVERLAP_MM = 0.05           # the middle of the fuzz sweep's range of overlaps


def spread_of(rmean):
    """the radius spread the packed tests use with a mean radius: 0.01 mm (0.005 for 0.35 mm grains, 0.02 for 0.6 mm)"""
    return {0.35: 0.005, 0.6: 0.02}.get(rmean, 0.01)


def tri_packing(lx, ly, rmean, spread=None, noise=0.003, margin=0.05, seed=7, shuffle=False, floor_push=False, n_max=None):
    """-> (r, x, y) in mm. The lattice fills the box left to right, bottom to top, `margin` from the walls (for discs of radius
    rmean); n_max keeps the first n_max grains of that order (whole bottom rows, then part of one). The draws, in this order,
    from numpy.random.default_rng(seed): the radii, the jitter (x and y of a grain together), the permutation (shuffle).
    floor_push: every third grain of the bottom row 2 um into the floor (y = r - 0.002), as test_gpu_contacts.shape_packing."""
    if spread is None:
        spread = spread_of(rmean)
    W, H = 0.1 * lx, 0.1 * ly
    pitch = 2.0 * rmean
    xs, ys = [], []
    row = 0
    while True:
        y = margin + rmean + row * pitch * SQ3_2
        if y + rmean + margin > H:
            break
        x = margin + rmean + (rmean if row % 2 else 0.0)
        while x + rmean + margin <= W:
            xs.append(x); ys.append(y)
            x += pitch
        row += 1
    x, y = np.array(xs), np.array(ys)
    if n_max is not None:
        x, y = x[:n_max], y[:n_max]
    n = len(x)
    rng = np.random.default_rng(seed)
    r = rmean + rng.uniform(-spread, spread, n)
    jit = rng.normal(0.0, noise, (n, 2))
    x, y = x + jit[:, 0], y + jit[:, 1]
    if floor_push and n:
        row0 = np.nonzero(y < y.min() + 0.1 * rmean)[0][::3]
        y[row0] = r[row0] - 0.002
    if shuffle:
        p = rng.permutation(n)
        r, x, y = r[p], x[p], y[p]
    return r, x, y


def tri_packing_m(lx, ly, rmean, **kw):
    """the same in metres: (r, x1, x2) as LbmDem and the oracle take them"""
    return samples.to_metres(*tri_packing(lx, ly, rmean, **kw))


def agitation(n, seed=7, scale=(0.05, 0.05, 30.0)):
    """(n, 9) kinematics with random velocities (positions and accelerations zero: the caller fills in the positions)"""
    k = np.zeros((n, 9))
    k[:, 3:6] = np.random.default_rng(seed).normal(0, 1, (n, 3)) * scale
    return k


def contact_scene():
    """the scene of the contact export test: 256 x 200, rmean 0.7, every third grain of the bottom row 2 um into the floor,
    random velocities and accelerations -> (lx, ly, r, x1, x2 in metres, the 9 kinematic columns)"""
    lx, ly = 256, 200
    r, x1, x2 = tri_packing_m(lx, ly, 0.7, floor_push=True)
    n = len(r)
    k = np.zeros((n, 9))
    k[:, 0], k[:, 1] = x1, x2
    rng = np.random.default_rng(n)
    k[:, 3:6] = rng.normal(0, 1, (n, 3)) * [0.3, 0.3, 40.0]
    k[:, 6:9] = rng.normal(0, 1, (n, 3)) * [5.0, 5.0, 3000.0]
    return lx, ly, r, x1, x2, k


def close_pairs(x, y, reach):
    """(m, 2) index pairs i < j with centres closer than `reach`, and their distances (all pairs: the scenes are small)"""
    n = len(x)
    out_i, out_j, out_d = [], [], []
    for a in range(0, n, 512):
        dx = x[a:a + 512, None] - x[None, :]
        dy = y[a:a + 512, None] - y[None, :]
        d = np.sqrt(dx * dx + dy * dy)
        i, j = np.nonzero(d < reach)
        keep = i + a < j
        out_i.append(i[keep] + a); out_j.append(j[keep]); out_d.append(d[i[keep], j[keep]])
    return np.stack([np.concatenate(out_i), np.concatenate(out_j)], 1), np.concatenate(out_d)


def touching_pairs(r, x, y):
    """(m, 2) pairs i < j whose discs overlap (dn = dist - r_i - r_j < 0, force_grains' test), and their overlaps -dn > 0"""
    r, x, y = (np.asarray(a, float) for a in (r, x, y))
    pairs, d = close_pairs(x, y, 2.0 * r.max())
    dn = d - r[pairs[:, 0]] - r[pairs[:, 1]]
    t = dn < 0
    return pairs[t], -dn[t]


def partner_counts(n, pairs):
    return np.bincount(pairs.reshape(-1), minlength=n)


def census(lx, ly, r, x, y):
    """the figures of the census table (LABBOOK.md) for a scene in mm"""
    n = len(r)
    pairs, over = touching_pairs(r, x, y)
    i, j = pairs[:, 0], pairs[:, 1]
    steep = np.abs(y[i] - y[j]) > np.abs(x[i] - x[j])
    return dict(grains=n, touching_pairs=len(pairs),
                frac_3_partners=float((partner_counts(n, pairs) >= 3).mean()) if n else 0.0,
                frac_steep=float(steep.mean()) if len(pairs) else 0.0,
                max_overlap=float(over.max()) if len(pairs) else 0.0,
                inside=bool(n and (x >= 0).all() and (x <= 0.1 * lx).all() and (y >= 0).all() and (y <= 0.1 * ly).all()))


def check_scene(lx, ly, r, x, y, what=""):
    """the conditions on the INPUTS of a packed test (mm); -> the census"""
    c = census(lx, ly, np.asarray(r, float), np.asarray(x, float), np.asarray(y, float))
    assert c["frac_3_partners"] >= MIN_FRAC_3_PARTNERS, (what, c)
    assert c["frac_steep"] >= MIN_FRAC_STEEP, (what, c)
    assert c["max_overlap"] <= MAX_OVERLAP_MM, (what, c)
    assert c["inside"], (what, c)
    return c


def check_scene_m(lx, ly, r, x1, x2, what=""):
    return check_scene(lx, ly, np.asarray(r) * 1e3, np.asarray(x1) * 1e3, np.asarray(x2) * 1e3, what)


def reduced_disc_partners(r, x, y, reduction):
    """per grain: how many other grains' reduced discs (radius reduction * r) meet its own"""
    r, x, y = (np.asarray(a, float) for a in (r, x, y))
    pairs, d = close_pairs(x, y, 2.0 * reduction * r.max())
    meet = d < reduction * (r[pairs[:, 0]] + r[pairs[:, 1]])
    return partner_counts(len(r), pairs[meet])


def cut_census(r, x, y, cut):
    """for a strip cut at x = cut (same unit as x): (touching pairs with centres on opposite sides, grains with two or more
    touching partners beyond the cut AND two or more on their own side)"""
    pairs, _ = touching_pairs(r, x, y)
    side = np.asarray(x) >= cut
    i, j = pairs[:, 0], pairs[:, 1]
    across = side[i] != side[j]
    n = len(r)
    beyond = np.bincount(np.concatenate([i[across], j[across]]), minlength=n)
    own = np.bincount(np.concatenate([i[~across], j[~across]]), minlength=n)
    return int(across.sum()), int(((beyond >= 2) & (own >= 2)).sum())
