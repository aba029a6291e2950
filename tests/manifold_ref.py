"""Numpy restatement of the one-shot hull-hull contact manifold (diy_gym_amd/csrc/dg_hull.h hull_manifold, DIYGym's
hull_manifold_points): same steps, same constants, same tie-breaks, in fp64.  The normal n (from B towards A) is an input -- the
kernel takes it from the pair's GJK / polytope contact, the tests from the device or from the closed form.

manifold(...) -> None when the pair keeps its single contact (a vertex on either side, crossed edges, nothing clipped below the
margin), else a list of (point, depth) in slot order (slot s is key feature s)."""
import numpy as np

TOL = 0.02      # DG_HULL_MANIFOLD_TOL (include/diygym_scene.h)
CAP = 8         # HH_MF_CAP: points per feature
CLIP = 16       # HH_MF_CLIP: vertices of a clipped polygon


def pseudo_angle(x, y):
    """Monotone stand-in for the angle of (x, y), in [0, 4), 0 along +x, counter-clockwise (hh_pseudo_angle)."""
    s = abs(x) + abs(y)
    if not s > 0:
        return 0.0
    p = y / s
    return 2.0 - p if x < 0 else (4.0 + p if y < 0 else p)


def basis(RA, n):
    """u: A's link-frame x axis (y if x is within ~26 degrees of n) projected on the plane normal to n; v = n x u."""
    a = RA[:, 0]
    if abs(a @ n) > 0.9:
        a = RA[:, 1]
    u = a - n * (a @ n)
    u = u / np.sqrt(u @ u)
    return u, np.cross(n, u)


def feature(pts, R, t, d, tol, u, v):
    """Points of the hull (link frame pts, pose R, t) within tol of its extreme along the world direction d, at most CAP: the
    extreme point (lowest index on a tie), then the lowest indices; ordered by angle about their centroid; and the extreme's
    support value."""
    dl = R.T @ d
    proj = pts @ dl
    ks = int(np.argmax(proj)); s = proj[ks]
    idx = []
    for k in range(len(pts)):
        if (k == ks or len(idx) < CAP - (1 if k < ks else 0)) and proj[k] >= s - tol:
            idx.append(k)
    X = np.array([R @ pts[k] + t for k in idx])
    c = X.mean(0)
    ang = [pseudo_angle((x - c) @ u, (x - c) @ v) for x in X]
    m = len(X)
    rank = [sum(1 for j in range(m) if ang[j] < ang[i] or (ang[j] == ang[i] and j < i)) for i in range(m)]
    out = np.zeros_like(X)
    for i in range(m):
        out[rank[i]] = X[i]
    return out, s


def manifold(pa, RA, ta, pb, RB, tb, n, rad_a, rad_b, margin, hull_margin, npts=4):
    """Hull A (points pa in its link frame, pose RA, ta) against hull B; n from B towards A.  Coordinates relative to A's origin
    inside, world coordinates out."""
    pa, pb, RA, RB = (np.asarray(x, np.float64) for x in (pa, pb, RA, RB))
    ta, tb, n = (np.asarray(x, np.float64) for x in (ta, tb, n))
    tBA = tb - ta
    u, v = basis(RA, n)
    FA, sA = feature(pa, RA, np.zeros(3), -n, TOL * rad_a, u, v)
    FB, sB = feature(pb, RB, tBA, n, TOL * rad_b, u, v)
    hA, hB = -sA, sB + tBA @ n
    ma, mb = len(FA), len(FB)
    if ma < 2 or mb < 2:
        return None
    if ma == 2 and mb == 2:
        ea, eb = FA[1] - FA[0], FB[1] - FB[0]
        cx = np.cross(ea, eb)
        if cx @ cx > TOL * TOL * (ea @ ea) * (eb @ eb):
            return None
    refA = ma >= 3 or mb < 3
    C, S = (FA, FB) if refA else (FB, FA)
    href, sgn = (hA, -1.0) if refA else (hB, 1.0)
    mc = len(C)
    if mc >= 3:
        planes = [(C[j], np.cross(n, C[(j + 1) % mc] - C[j])) for j in range(mc)]
    else:
        planes = [(C[0], C[1] - C[0]), (C[1], C[0] - C[1])]
    if len(S) == 2:
        p0, dr = S[0], S[1] - S[0]
        t0, t1 = 0.0, 1.0
        for q, d in planes:
            f0, fd = (p0 - q) @ d, dr @ d
            if fd == 0:
                if f0 < 0:
                    t1 = -1.0
            elif fd > 0:
                t0 = max(t0, -f0 / fd)
            else:
                t1 = min(t1, -f0 / fd)
        poly = [p0 + dr * t0, p0 + dr * t1] if t0 <= t1 else []
    else:  # Sutherland-Hodgman
        poly = list(S)
        for q, d in planes:
            if not poly:
                break
            out = []
            prev = poly[-1]
            fp = (prev - q) @ d
            for cur in poly:
                fc = (cur - q) @ d
                if (fc >= 0) != (fp >= 0) and len(out) < CLIP:
                    out.append(prev + (cur - prev) * (fp / (fp - fc)))
                if fc >= 0 and len(out) < CLIP:
                    out.append(cur)
                prev, fp = cur, fc
            poly = out
    # C's feature plane: through its centroid, normal = the polygon's area vector (Newell); an edge: the plane through it nearest
    # to normal to n; leaning more than ~26 degrees from n: the plane normal to n through C's extreme
    c0 = C.mean(0)
    if mc >= 3:
        nc = sum(np.cross(C[j] - c0, C[(j + 1) % mc] - c0) for j in range(mc))
    else:
        e = C[1] - C[0]; ee = e @ e
        nc = n - e * ((e @ n) / ee) if ee > 1e-20 else n.copy()
    dn = n @ nc
    if not (dn * dn >= 0.81 * (nc @ nc)) or dn == 0:
        nc, c0, dn = n.copy(), n * href, 1.0
    K, D = [], []
    for x in poly:
        t = -((x - c0) @ nc) / dn
        sep = -sgn * t
        depth = sep - 2 * hull_margin
        if depth < margin:
            K.append(x + n * (0.5 * t)); D.append(depth)
    if not K:
        return None
    nk = len(K)
    i0 = 0
    for i in range(1, nk):
        if D[i] < D[i0]:
            i0 = i
    chosen = [i0]
    x0 = K[i0]
    if npts >= 2 and nk >= 2:
        chosen.append(_argmax([(K[i] - x0) @ (K[i] - x0) for i in range(nk)], chosen))
    if npts >= 3 and nk >= 3:
        x1 = K[chosen[1]]
        chosen.append(_argmax([np.sum(np.cross(x1 - x0, K[i] - x0) ** 2) for i in range(nk)], chosen))
    if npts >= 4 and nk >= 4:
        x1, x2 = K[chosen[1]], K[chosen[2]]
        o = -1.0 if np.cross(x1 - x0, x2 - x0) @ n >= 0 else 1.0
        sc = [max(o * (np.cross(x1 - x0, x - x0) @ n), o * (np.cross(x2 - x1, x - x1) @ n), o * (np.cross(x0 - x2, x - x2) @ n)) for x in K]
        chosen.append(_argmax(sc, chosen))
    P = [K[i] for i in chosen]
    cm = np.mean(P, axis=0)
    g = [pseudo_angle((x - cm) @ u, (x - cm) @ v) for x in P]
    m = len(P)
    slot = [sum(1 for j in range(m) if g[j] < g[c] or (g[j] == g[c] and j < c)) for c in range(m)]
    res = [None] * m
    for c in range(m):
        res[slot[c]] = (P[c] + ta, D[chosen[c]])
    return res


def _argmax(scores, exclude):
    best, bi = -3.0e38, -1
    for i, s in enumerate(scores):
        if i not in exclude and s > best:
            best, bi = s, i
    return bi


def box_points(half):
    """The 8 corners of a box of half extents `half` (the order scene.py's box hulls use does not matter here)."""
    hx, hy, hz = half
    return np.array([[sx * hx, sy * hy, sz * hz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64)


def rot_z(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def rot_x(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])
