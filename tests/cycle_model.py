"""The level transfers and the corrected V-cycle (cycle = 1) from vertex coordinates: an independent model.

Plain numpy in np.longdouble, on top of tests/face_model.py. Like it, this module shares one thing with the
code under test, the storage layout (`str_info` / `splitting`). It does not know which four fine
sub-elements make up a coarse one, nor which local node of a child sits on which coarse vertex or edge:
the code under test takes both from element_conversion and hard-coded child / node tables, the model
finds them by geometry.

  - The parent of a fine sub-element is the coarse sub-element of the same un_ele whose triangle
    contains the fine centroid (all three barycentric coordinates > 0, exactly one match).
  - lam[e, i, j] is the barycentric coordinate of fine node i with respect to the parent's node j: 0,
    1/2 or 1. The P1 interpolant of a coarse field y at that node is sum_j lam[e, i, j] y[parent(e), j].
  - The restrictor is the reference's (splitting.F90:10-32): component j of coarse sub-element c is the
    mean of the three residual components of the child that sits on c's vertex j. The centre child is
    never read and nothing is scaled by an area. These are not the weights of the interpolation's
    transpose; the corrected cycle keeps them by design (it fixes the cycle's composition, not its
    transfer operators).

`corrected_cycle` composes them with FaceModel's sweeps into one corrected V-cycle: fresh residuals
b - A x restricted on the way down, coarse levels started from zero, the interpolated correction added
before the post-smoothing, n_coarse smoother calls (or the direct solve) on the coarsest level.
"""
import copy

import numpy as np

from face_model import LD, splitting


def _cross(u, v):
    return u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]


def barycentric(T, p):
    """the barycentric coordinates (..., 3) of the points p (..., 2) in the triangles T (..., 3, 2)"""
    a, b, c = T[..., 0, :], T[..., 1, :], T[..., 2, :]
    den = _cross(b - a, c - a)
    return np.stack([_cross(b - p, c - p), _cross(c - p, a - p), _cross(a - p, b - p)], axis=-1) / den[..., None]


class TransferModel:
    """Fine level `level` <-> coarse level `level + 1` of one mesh. X: the un_eles' coordinates, flat
    (2, 3, U) column-major as oracle_lib.Mesh.X, or (U, 3, 2)."""

    def __init__(self, X, n_split, level):
        X = np.asarray(X, np.float64)
        if X.ndim == 1:
            X = X.reshape(-1, 3, 2)
        self.level = level
        Pf, Pc = splitting(X, n_split - level + 1), splitting(X, n_split - level)
        U, nf, nc = Pf.shape[0], Pf.shape[1], Pc.shape[1]
        self.U, self.nf, self.nc = U, nf, nc
        ar = np.arange(U)[:, None]
        # ---- parents. A point of un_ele u is X3 + a e1 + b e2 with e1 = (X1 - X3) / n, e2 = (X2 - X3) / n, n the
        # coarse sub-elements along an edge: (floor a, floor b) names a parallelogram of the coarse lattice,
        # which holds at most two coarse triangles. Only those two are tried for a fine centroid inside it.
        n = 2 ** (n_split - level)
        XL = X.astype(LD)
        e1, e2 = (XL[:, None, 0] - XL[:, None, 2]) / n, (XL[:, None, 1] - XL[:, None, 2]) / n

        def cell(p):
            d = p - XL[:, None, 2]
            a, b = _cross(d, e2) / _cross(e1, e2), _cross(e1, d) / _cross(e1, e2)
            return np.floor(a).astype(np.int64) * n + np.floor(b).astype(np.int64)

        cc = cell(Pc.mean(axis=2))
        assert cc.min() >= 0 and cc.max() < n * n
        order = np.argsort(cc, axis=1, kind="stable")
        sc = np.take_along_axis(cc, order, axis=1)
        second = np.zeros(sc.shape, np.int64)
        second[:, 1:] = sc[:, 1:] == sc[:, :-1]
        assert nc < 3 or (sc[:, 2:] != sc[:, :-2]).all(), "three coarse triangles in one lattice cell"
        cand = np.full((U, n * n, 2), -1, np.int64)
        cand[ar, sc, second] = order
        cf = Pf.mean(axis=2)
        c2 = cand[ar, cell(cf)]                                     # (U, nf, 2)
        inside = np.stack([(barycentric(Pc[ar, np.maximum(c2[..., t], 0)], cf) > 0).all(axis=-1) & (c2[..., t] >= 0)
                           for t in range(2)], axis=-1)
        assert (inside.sum(axis=-1) == 1).all(), "a fine centroid is not in exactly one coarse triangle"
        self.parent = np.where(inside[..., 0], c2[..., 0], c2[..., 1])   # (U, nf)
        assert (np.stack([np.bincount(p, minlength=nc) for p in self.parent]) == 4).all()
        # ---- the P1 weights of every fine node in its parent
        Pp = Pc[ar, self.parent]                                     # (U, nf, 3, 2)
        lam = np.stack([barycentric(Pp, Pf[:, :, i]) for i in range(3)], axis=2)   # (U, nf, fine node, coarse node)
        r = np.rint(lam * 2) / 2
        assert np.abs(lam - r).max() < 1e-9 and r.min() >= 0 and r.max() <= 1
        self.lam = r.astype(LD)
        # ---- the child on each coarse vertex
        self.corner = np.full((U, nc, 3), -1, np.int64)
        for j in range(3):
            u, f = np.nonzero((self.lam[..., j] == 1).any(axis=-1))
            count = np.zeros((U, nc), np.int64)
            np.add.at(count, (u, self.parent[u, f]), 1)
            assert (count == 1).all(), "the child on a coarse vertex is not unique"
            self.corner[u, self.parent[u, f], j] = f
        s = np.sort(self.corner, axis=-1)
        assert (s[..., 1:] != s[..., :-1]).all()

    def interpolate(self, y):
        """the P1 interpolant of the coarse field y (3, nc, U) at the fine nodes, (3, nf, U)"""
        yp = np.asarray(y, LD).transpose(2, 1, 0)[np.arange(self.U)[:, None], self.parent]   # (U, nf, 3)
        return np.einsum("ufij,ufj->ufi", self.lam, yp).transpose(2, 1, 0)

    def restrict(self, r):
        """the coarse RHS (3, nc, U) from the fine residual r (3, nf, U): per coarse vertex the mean of the three
        components on its corner child (splitting.F90:10-32). The centre child is never read and there is no area
        scaling; cycle = 1 keeps these weights by design."""
        rs = np.asarray(r, LD).transpose(2, 1, 0)
        mean = (rs[..., 0] + rs[..., 1] + rs[..., 2]) / 3                                   # (U, nf)
        return mean[np.arange(self.U)[:, None, None], self.corner].transpose(2, 1, 0)

    # ---- deliberately wrong transfers: what a wrong child or node table would do
    def mutant(self, kind):
        m = copy.copy(self)
        if kind == "corners_rotated":        # coarse vertex j reads the child on vertex j + 1
            m.corner = np.roll(self.corner, -1, axis=-1)
        elif kind == "injection":            # fine node i takes the parent's node i instead of the interpolant
            m.lam = np.broadcast_to(np.eye(3, dtype=LD), self.lam.shape).copy()
        elif kind == "nodes_swapped":        # coarse nodes 0 and 1 exchanged in the interpolation
            m.lam = self.lam[..., [1, 0, 2]]
        else:
            raise ValueError(kind)
        return m


def corrected_cycle(models, transfers, x1, rhs1, n_smooth, n_coarse, solver, op, coarse_solver=0):
    """One corrected V-cycle from the level-1 iterate x1 and RHS rhs1. models: {level: FaceModel} for
    1..L; transfers: {level: TransferModel} for 1..L-1. Returns (x, b, res): the iterate and the RHS of every
    level after the cycle, and the residuals b - A x -- res[l] for l < L as restricted on the way down,
    res["final"] the level-1 residual after the cycle."""
    L = len(models)
    x, b, res = {1: np.asarray(x1, LD)}, {1: np.asarray(rhs1, LD)}, {}

    def smooth(l, calls):
        md = models[l]
        for _ in range(calls * n_smooth):
            x[l] = md.sweep(x[l], b[l], solver) if op == 1 else md.sweep0(x[l], b[l])

    def residual(l):
        md = models[l]
        return b[l] - (md.apply(x[l]) if op == 1 else md.apply0(x[l]))

    for l in range(1, L):
        if l > 1:
            x[l] = np.zeros_like(b[l])
        smooth(l, 1)
        res[l] = residual(l)
        b[l + 1] = transfers[l].restrict(res[l])
    if L == 1:
        smooth(1, 1)
    else:
        x[L] = np.zeros_like(b[L])
        if coarse_solver == 1:
            assert op == 0
            x[L] = models[L].solve0(b[L])
        else:
            smooth(L, n_coarse)
    for l in range(L - 1, 0, -1):
        x[l] = x[l] + transfers[l].interpolate(x[l + 1])
        smooth(l, 1)
    res["final"] = residual(1)
    return x, b, res


def cycle_diffs(state, x, b, res):
    """The error figures of a state ({"tnew_L1": .., "RHS_L1": .., "res_L1": .., ..}, Oracle.state() or the HIP
    handle's) after a cycle against the model's (x, b, res): tnew-like fields against max |model tnew_L1|;
    RHS and residual fields against the largest |value| among the model's RHS and residual fields of all
    levels of that cycle (from a random start |res_1| is about 1e3 |RHS_1| at P2: a ratio to |RHS_1| alone
    would read three digits worse than the arithmetic is). Compared: tnew_l and RHS_l on every level, res_l
    for 1 < l < L, and the final res_1, which the state keeps in place of the one restricted on the way down
    (that one is seen through RHS_2). Returns {"tnew": .., "RHS": .., "res": ..}."""
    L = len(x)
    tscale = np.abs(x[1]).max()
    rscale = max(np.abs(v).max() for v in list(b.values()) + list(res.values()))

    def dist(key, model, scale):
        return float(np.abs(np.asarray(state[key], LD) - model).max() / scale)

    out = {"tnew": max(dist(f"tnew_L{l}", x[l], tscale) for l in range(1, L + 1)),
           "RHS": max(dist(f"RHS_L{l}", b[l], rscale) for l in range(1, L + 1)),
           "res": max([dist("res_L1", res["final"], rscale)] +
                      [dist(f"res_L{l}", res[l], rscale) for l in range(2, L)])}
    return out
