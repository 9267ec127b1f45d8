"""The face-coupled operator (op = 1) assembled from vertex coordinates: an independent model.

Plain numpy in np.longdouble. It shares ONE thing with the code under test, the storage layout:
which sub-element of an un_ele, and which of its local nodes, sits where in a level field
(3, nsub, U). That is get_str_info / get_splitting (Msh2Tri.F90:32-107), restated in `str_info`
and `splitting` below as the layout's definition. Everything else comes from the coordinates of the
sub-elements' vertices:

  - the P1 mass matrix area/12 [[2,1,1],[1,2,1],[1,1,2]], the stiffness k area grad phi_i . grad phi_j
    and the lumped mass area/3 of every sub-element;
  - faces matched by their midpoints (a hash of the quantised midpoint) -- never through Neig,
    fNeig, Dir or str_neig; the neighbour's values are taken at the nodes whose coordinates
    coincide with the face's;
  - the face matrix k/delta |e|/6 [[2,1],[1,2]], delta the distance of the two centroids, at a
    domain boundary the distance from the centroid to the face's midpoint;
  - boundary data at a domain boundary: sin(x + y) at the face's nodes on level 1, zero on the
    coarser levels (they carry the error equation);
  - the diagonal D_i = ml_i/dt + Kd_ii + sum over the faces at node i of 2 w_f.

Level 1's source term is the reference's in-place cascade (get_RHS, transport_tri_semi.F90:452-464,
593): with f = -2k sin(x + y) at the nodes, s'_0 = M_0. f, then s'_1 = M_10 s'_0 + M_11 f_1 +
M_12 f_2 and s'_2 = M_20 s'_0 + M_21 s'_1 + M_22 f_2. It is NOT M f (12 % off at dt = 0.05);
`source_level1` restates the cascade, and every method that needs s' also takes it as an input.

The block-diagonal operator of op = 0 is here too (A0 = M/dt + k K1, D0 = ml/dt + k diag K1, its sweep
and its exact solve per sub-element). One level at a time is all this module knows: what joins the
levels -- the restrictor, the P1 interpolation -- and the corrected V-cycle composed from these sweeps
are in tests/cycle_model.py, found from coordinates in the same way and held against the oracle and the
HIP path in tests/test_cycle_model.py.

Fields go in and come out in the reference's shape (3, nsub, U); results are np.longdouble.
"""
import copy

import numpy as np

LD = np.longdouble
FACES = ((0, 2), (2, 1), (1, 0))   # the three edges of a triangle as pairs of local nodes


# ---------------------------------------------------------------- the storage layout
def str_info(i_split):
    """(irow, ipos) of the sub-elements 1..4^i_split in storage order: row r = 1.. holds
    2^(i_split+1) - 1 - 2 (r - 1) sub-elements, ipos counts along the row; odd ipos: an up
    sub-element, even: a down one."""
    irow, ipos = [], []
    for r in range(1, 2 ** i_split + 1):
        n = 2 ** (i_split + 1) - 1 - 2 * (r - 1)
        irow += [r] * n
        ipos += list(range(1, n + 1))
    return np.array(irow), np.array(ipos)


def splitting(X, i_split):
    """vertex coordinates (U, nsub, 3, 2) of every sub-element's local nodes from the un_eles'
    X (U, 3, 2): the un_ele is cut along v1 = (X1 - X3) / 2^i_split and v2 = (X2 - X3) / 2^i_split"""
    X = np.asarray(X, LD)
    p = LD(2 ** i_split)
    x3 = X[:, None, 2, :]
    v1 = ((X[:, 0, :] - X[:, 2, :]) / p)[:, None, :]
    v2 = ((X[:, 1, :] - X[:, 2, :]) / p)[:, None, :]
    irow, ipos = str_info(i_split)
    r = irow.astype(LD)[None, :, None]
    h = (ipos // 2).astype(LD)[None, :, None]
    up = np.stack([x3 + (r - 1) * v2 + (h + 1) * v1, x3 + r * v2 + h * v1, x3 + (r - 1) * v2 + h * v1], axis=2)
    down = np.stack([x3 + r * v2 + (h - 1) * v1, x3 + (r - 1) * v2 + h * v1, x3 + r * v2 + h * v1], axis=2)
    return np.where((ipos % 2 == 1)[None, :, None, None], up, down)


# ---------------------------------------------------------------- face matching by coordinates
def _match_midpoints(mid, q):
    """partner[j] = the other face whose midpoint coincides with face j's (within q), -1 if none.
    Midpoints are hashed on a grid of pitch q; faces left alone try the grid shifted by half a
    pitch in x, y and both, so that a pair split by a cell border still meets."""
    n = len(mid)
    partner = np.full(n, -1, np.int64)
    for off in ((0.0, 0.0), (0.5, 0.0), (0.0, 0.5), (0.5, 0.5)):
        idx = np.flatnonzero(partner < 0)
        if not idx.size:
            break
        cell = np.floor(mid[idx] / q + np.array(off)).astype(np.int64)
        _, inv, cnt = np.unique(cell, axis=0, return_inverse=True, return_counts=True)
        inv = inv.reshape(-1)
        assert cnt.max() <= 2, "more than two faces share a midpoint"
        order = np.argsort(inv, kind="stable")
        first = np.flatnonzero(cnt[inv[order]] == 2)[::2]
        a, b = idx[order[first]], idx[order[first + 1]]
        partner[a], partner[b] = b, a
    return partner


class FaceModel:
    """One level of one mesh. X: the un_eles' coordinates, flat (2, 3, U) column-major as
    oracle_lib.Mesh.X, or (U, 3, 2)."""

    def __init__(self, X, n_split, level, dt, k, omega):
        X = np.asarray(X, np.float64)
        if X.ndim == 1:
            X = X.reshape(-1, 3, 2)
        self.dt, self.k, self.omega, self.level = LD(dt), LD(k), LD(omega), level
        self.i_split = n_split - level + 1
        P = self.P = splitting(X, self.i_split)
        U, nsub = P.shape[:2]
        self.U, self.nsub = U, nsub
        self.up = str_info(self.i_split)[1] % 2 == 1
        e = np.stack([P[:, :, (i + 2) % 3] - P[:, :, (i + 1) % 3] for i in range(3)], axis=2)   # opposite edges
        d1, d2 = P[:, :, 1] - P[:, :, 0], P[:, :, 2] - P[:, :, 0]
        area = self.area = np.abs(d1[..., 0] * d2[..., 1] - d1[..., 1] * d2[..., 0]) / 2
        self.M = area[..., None, None] / 12 * (np.ones((3, 3), LD) + np.eye(3, dtype=LD))
        # grad phi_i = the opposite edge turned by 90 degrees / (2 area): the dot product keeps e_i . e_j
        self.K1 = np.einsum("usid,usjd->usij", e, e) / (4 * area[..., None, None])
        self.ml = area[..., None] / 3 * np.ones(3, LD)
        # ---- faces
        cen = P.mean(axis=2)
        mid = np.stack([(P[:, :, a] + P[:, :, b]) / 2 for a, b in FACES], axis=2)          # (U, nsub, 3, 2)
        length = np.stack([np.linalg.norm(P[:, :, a] - P[:, :, b], axis=-1) for a, b in FACES], axis=2)
        q = float(length.min()) * 1e-3
        partner = _match_midpoints(mid.reshape(-1, 2).astype(np.float64), q)
        self.interior = (partner >= 0).reshape(U, nsub, 3)
        pe = np.where(partner >= 0, partner // 3, 0)           # flat (u, sub-element) of the neighbour
        self.nb = pe.reshape(U, nsub, 3)
        self.inner = self.interior & (self.nb // nsub == np.arange(U)[:, None, None])
        Pn = P.reshape(-1, 3, 2)[pe].reshape(U, nsub, 3, 3, 2)  # the neighbour's nodes, per face
        self.nb_node = np.zeros((U, nsub, 3, 2), np.int64)      # its local nodes at my face nodes a, b
        for f, ab in enumerate(FACES):
            for t, a in enumerate(ab):
                d = np.linalg.norm(Pn[:, :, f] - P[:, :, None, a], axis=-1)   # (U, nsub, 3)
                self.nb_node[:, :, f, t] = d.argmin(axis=-1)
                assert (d.min(axis=-1)[self.interior[:, :, f]] <= 1e-9 * length[:, :, f][self.interior[:, :, f]]).all()
        delta = np.where(self.interior, np.linalg.norm(cen[:, :, None] - cen.reshape(-1, 2)[pe].reshape(U, nsub, 3, 2),
                                                       axis=-1),
                         np.linalg.norm(cen[:, :, None] - mid, axis=-1))
        self.w1 = length / delta / 6                             # the face weight without k
        # boundary data at my face nodes: sin(x + y) on level 1, zero on the error-equation levels
        g = np.stack([np.stack([np.sin(P[:, :, a, 0] + P[:, :, a, 1]) for a in ab], axis=-1) for ab in FACES], axis=2)
        self.g = g if level == 1 else np.zeros_like(g)

    def with_params(self, dt, k, omega):
        """the same geometry (shared, read-only) at other parameters"""
        m = copy.copy(self)
        m.dt, m.k, m.omega = LD(dt), LD(k), LD(omega)
        return m

    # ---- helpers: fields as (U, nsub, 3) inside, (3, nsub, U) outside
    @staticmethod
    def _in(x):
        return np.asarray(x, LD).transpose(2, 1, 0)

    @staticmethod
    def _out(x):
        return x.transpose(2, 1, 0)

    @property
    def w(self):
        return self.k * self.w1

    @property
    def D(self):
        """the diagonal the smoother divides by, (3, nsub, U)"""
        D = self.ml / self.dt + self.k * np.einsum("usii->usi", self.K1)
        D = D.copy()
        for f, (a, b) in enumerate(FACES):
            D[:, :, a] += 2 * self.w[:, :, f]
            D[:, :, b] += 2 * self.w[:, :, f]
        return self._out(D)

    def _neighbour_values(self, xi, xo, swap_outer):
        """(U, nsub, 3 faces, 2) the values facing my face nodes a, b"""
        fi, fo = xi.reshape(-1, 3), xo.reshape(-1, 3)
        y = np.where(self.inner[..., None], fi[self.nb[..., None], self.nb_node], fo[self.nb[..., None], self.nb_node])
        if swap_outer:
            y = np.where((self.interior & ~self.inner)[..., None], y[..., ::-1], y)
        return np.where(self.interior[..., None], y, self.g)

    def face_part(self, x, x_inner=None, x_outer=None, swap_outer=False):
        """sum over the faces of w_f [[2,1],[1,2]] (x_face - y_face), (3, nsub, U)"""
        xs = self._in(x)
        y = self._neighbour_values(xs if x_inner is None else self._in(x_inner),
                                   xs if x_outer is None else self._in(x_outer), swap_outer)
        ds = np.zeros_like(xs)
        for f, (a, b) in enumerate(FACES):
            w = self.w[:, :, f]
            ds[:, :, a] += w * (2 * xs[:, :, a] + xs[:, :, b] - 2 * y[:, :, f, 0] - y[:, :, f, 1])
            ds[:, :, b] += w * (xs[:, :, a] + 2 * xs[:, :, b] - y[:, :, f, 0] - 2 * y[:, :, f, 1])
        return self._out(ds)

    def apply(self, x, x_inner=None, x_outer=None, swap_outer=False):
        """A x = (M/dt + Kd) x + the face part. The neighbours inside the un_ele are read from x_inner
        and those across an un_ele face from x_outer (both default to x); at a domain boundary the
        boundary data stand in (so A is affine on level 1). swap_outer exchanges the two neighbour
        values of every face between un_eles: what a wrong Dir would do."""
        xs = self._in(x)
        vol = np.einsum("usij,usj->usi", self.M / self.dt + self.k * self.K1, xs)
        return self._out(vol) + self.face_part(x, x_inner, x_outer, swap_outer)

    def source_level1(self):
        """the cascaded source term s' (see the module docstring)"""
        assert self.level == 1
        P, M = self.P, self.M
        s = [-(2 * self.k) * np.sin(P[:, :, i, 0] + P[:, :, i, 1]) for i in range(3)]
        for i in range(3):
            s[i] = M[:, :, i, 0] * s[0] + M[:, :, i, 1] * s[1] + M[:, :, i, 2] * s[2]
        return self._out(np.stack(s, axis=-1))

    def rhs_level1(self, told, source=None):
        """level 1's right-hand side M told / dt + s'"""
        assert self.level == 1
        s = self.source_level1() if source is None else np.asarray(source, LD)
        return self._out(np.einsum("usij,usj->usi", self.M, self._in(told)) / self.dt) + s

    def residual(self, x, rhs, **kw):
        """A x - rhs (level 1: rhs = rhs_level1(told, s'))"""
        return self.apply(x, **kw) - np.asarray(rhs, LD)

    def sweep(self, x, rhs, solver):
        """one smoother sweep x + omega/D (rhs - A x): Jacobi for solver 1; red-black for solver 3 -- the up
        sub-elements (odd ipos) first, then the down ones, the neighbours across un_ele faces read from the
        snapshot taken at the sweep's start for both colours, the inner ones from the current iterate"""
        x0 = np.asarray(x, LD)
        b = np.asarray(rhs, LD)
        wD = self.omega / self.D
        if solver == 1:
            return x0 + wD * (b - self.apply(x0))
        assert solver == 3
        x1 = x0.copy()
        for colour in (self.up, ~self.up):
            step = wD * (b - self.apply(x1, x_inner=x1, x_outer=x0))
            x1[:, colour, :] += step[:, colour, :]
        return x1

    # ---- the volume operator alone (op = 0): block-diagonal, one 3 x 3 block per sub-element
    @property
    def A0(self):
        """the blocks M/dt + k K1, (U, nsub, 3, 3)"""
        return self.M / self.dt + self.k * self.K1

    @property
    def D0(self):
        """the diagonal of op = 0's smoother, ml/dt + k diag(K1), (3, nsub, U)"""
        return self._out(self.ml / self.dt + self.k * np.einsum("usii->usi", self.K1))

    def apply0(self, x):
        """A0 x"""
        return self._out(np.einsum("usij,usj->usi", self.A0, self._in(x)))

    def sweep0(self, x, rhs):
        """one sweep x + omega/D0 (rhs - A0 x) of op = 0: Jacobi within a sub-element, and nothing couples two
        sub-elements, so solver 1 and solver 3 are the same sweep"""
        x0 = np.asarray(x, LD)
        return x0 + self.omega / self.D0 * (np.asarray(rhs, LD) - self.apply0(x0))

    def solve0(self, rhs):
        """A0^-1 rhs per sub-element by Cramer's rule in long double (numpy's solve has no long double)"""
        A, b = self.A0, self._in(rhs)

        def det(m):
            return (m[..., 0, 0] * (m[..., 1, 1] * m[..., 2, 2] - m[..., 1, 2] * m[..., 2, 1])
                    - m[..., 0, 1] * (m[..., 1, 0] * m[..., 2, 2] - m[..., 1, 2] * m[..., 2, 0])
                    + m[..., 0, 2] * (m[..., 1, 0] * m[..., 2, 1] - m[..., 1, 1] * m[..., 2, 0]))

        d, cols = det(A), []
        for i in range(3):
            Ai = A.copy()
            Ai[..., :, i] = b
            cols.append(det(Ai) / d)
        return self._out(np.stack(cols, axis=-1))


def rel_diff(got, model):
    """max |got - model| / max |model|, the figure every bound of the model tests is stated in"""
    model = np.asarray(model, LD)
    return float(np.abs(np.asarray(got, LD) - model).max() / max(np.abs(model).max(), LD(1e-300)))


def coordinate_map(Pa, Pb):
    """For two numberings of the same triangles (vertex coordinates (U, nsub, 3, 2) from `splitting`): idx
    (U, nsub, 3) such that node (u, e, i) of a is node idx[u, e, i] of b's fields flattened as (U, nsub, 3).
    Un_eles, then sub-elements, are matched by their centroids, nodes by their coordinates."""
    U, nsub = Pa.shape[:2]
    ca, cb = Pa.mean(axis=2), Pb.mean(axis=2)
    h = np.linalg.norm(Pa[:, :, 0] - Pa[:, :, 1], axis=-1).min()
    idx = np.empty((U, nsub, 3), np.int64)
    for u in range(U):
        d = np.linalg.norm(cb.mean(axis=1) - ca[u].mean(axis=0), axis=-1)
        v = int(d.argmin())
        assert d[v] <= 1e-9 * h
        d = np.linalg.norm(ca[u][:, None] - cb[v][None], axis=-1)          # (nsub, nsub)
        e = d.argmin(axis=1)
        assert (d.min(axis=1) <= 1e-9 * h).all()
        d = np.linalg.norm(Pa[u][:, :, None] - Pb[v][e][:, None, :], axis=-1)   # (nsub, 3, 3)
        assert (d.min(axis=2) <= 1e-9 * h).all()
        idx[u] = (v * nsub + e)[:, None] * 3 + d.argmin(axis=2)
    assert len(np.unique(idx)) == idx.size
    return idx


def renumbered(field_b, idx):
    """b's field (3, nsub, U) in a's numbering"""
    fb = np.asarray(field_b).transpose(2, 1, 0).reshape(-1)
    return fb[idx].transpose(2, 1, 0)
