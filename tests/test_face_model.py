"""The oracle's face-coupled operator (op = 1) against a model assembled from coordinates.

oracle/pamg_oracle.c defines op = 1 (the reference cannot run its surface terms), and every GPU form
is held to it bit for bit: nothing outside the project said what its values should be. face_setup
takes each face weight from the first sub-element that has the face and checks the slot geometry
against coordinates for slot 1 only. tests/face_model.py assembles the same operator from the
sub-elements' vertex coordinates alone (faces matched by midpoint, neighbour values by coinciding
nodes) and shares only the storage layout with the code under test.

The meshes are the six small fixtures and the three renumbered variants (tests/mesh_variants.py),
which together show all 18 (face, fNeig, Dir) triples of an interior face; the fixtures alone show 14.
Guards keep the comparison from passing vacuously: the face terms are a large part of A x where it
counts, a sweep moves the iterate, the model is sensitive to what Dir encodes, and the topology
cases are really reached. The whole cycle is pinned independently of any numbering by running the
oracle on a fixture and on its variant from a source term defined by coordinates.
"""
import os

import numpy as np
import pytest

import face_model as F
import goldens
import mesh_variants as V
import oracle_lib as O
from test_parameters import SETS, drive

FIXTURES = ["2_unele_test.msh", "900_ele.msh", "irregular.msh", "one_tri.msh", "test_sn2.msh", "untitled8.msh"]
VARIANTS = sorted(V.VARIANTS)
S, L = 3, 3
BOUND = 1e-12       # of the model field's maximum: a hundredth of the project's 1e-10 bar
CYCLE_BOUND = 1e-10  # the project's bar


def path_of(mesh):
    return os.path.join(goldens.MESHES, mesh)


_MESHES, _MODELS = {}, {}


def mesh_of(name):
    if name not in _MESHES:
        _MESHES[name] = O.read_msh(path_of(name))
    return _MESHES[name]


def model_of(name, n_split, level, pset):
    """the level's geometry, built once per mesh and shared by the parameter sets"""
    key = (name, n_split, level)
    if key not in _MODELS:
        _MODELS[key] = F.FaceModel(mesh_of(name).X, n_split, level, dt=1.0, k=1.0, omega=1.0)
    p = SETS[pset]
    return _MODELS[key].with_params(p["dt"], p["k"], p["omega"])


def physics(pset):
    return {k: SETS[pset][k] for k in ("dt", "k", "omega")}


@pytest.mark.parametrize("pset", ["default", "P1", "P2"])
@pytest.mark.parametrize("mesh", FIXTURES + VARIANTS)
def test_oracle_operator_is_the_coordinate_model(mesh, pset):
    """get_residual, level 1's source term and RHS, and one smoother call (n_smooth = 1) of solvers 1 and 3,
    on every level of (mesh, S 3, L 3), arith = 0, from random tnew / told / RHS: within 1e-12 of the model
    field's maximum. Measured maxima over the three parameter sets (residual / RHS / source / sweep):
      2_unele_test 2.7e-16 / 2.4e-16 / 2.4e-16 / 5.1e-16    900_ele      3.6e-14 / 1.6e-15 / 6.9e-15 / 3.2e-14
      irregular    4.6e-15 / 3.4e-16 / 3.7e-16 / 3.5e-15    one_tri      6.9e-16 / 2.3e-16 / 1.8e-16 / 3.8e-16
      test_sn2     1.4e-15 / 1.6e-16 / 2.0e-16 / 1.5e-15    untitled8    4.7e-15 / 2.6e-16 / 3.6e-16 / 3.1e-15
      untitled8_rn 3.1e-15 / 2.7e-16 / 3.4e-16 / 5.7e-15    irregular_rn 1.1e-14 / 2.7e-16 / 3.3e-16 / 3.0e-15
      test_sn2_rn  1.1e-15 / 1.8e-16 / 2.0e-16 / 1.7e-15
    (900_ele at P2 is the worst: its un_eles are small against their distance from the origin, so the oracle's
    fp64 coordinates carry the largest relative error, and k / dt weighs the terms built from them most.) The
    bound is 28 times that worst value and a hundredth of the project's 1e-10 bar. At P2 the model's face part is
    at least 0.25 of max |A x| on every level (measured: at least 0.46; at the default dt the mass term hides it,
    down to 0.00), a sweep moves the iterate by more than 0.1 at every set (measured: at least 0.51), and the
    model with the two neighbour values of every face between un_eles swapped is more than 1e-3 away from the
    oracle at P2 (measured: at least 0.059), so the comparison sees what Dir encodes."""
    m = mesh_of(mesh)
    rng = np.random.default_rng(20251019)
    worst = dict(residual=0.0, rhs=0.0, source=0.0, sweep=0.0)
    share, moved, swapped = np.inf, np.inf, np.inf
    oracles = {solver: O.Oracle(m, S, L, n_smooth=1, solver=solver, op=1, arith=0, **physics(pset))
               for solver in (1, 3)}
    for l in range(1, L + 1):
        md = model_of(mesh, S, l, pset)
        x, xo, b = (rng.uniform(-1, 1, (3, md.nsub, m.U)) for _ in range(3))
        for solver, o in oracles.items():
            for what, v in ((O.TNEW, x), (O.TOLD, xo), (O.RHS, b)):
                o.set(what, l, v)
            o.get_residual(l)
            rhs = b
            if l == 1:   # get_residual assembles level 1's RHS itself
                rhs = md.rhs_level1(xo)
                worst["source"] = max(worst["source"], F.rel_diff(o.get(O.SOURCE, 1), md.source_level1()))
                worst["rhs"] = max(worst["rhs"], F.rel_diff(o.get(O.RHS, 1), rhs))
            res = o.get(O.RES, l)
            worst["residual"] = max(worst["residual"], F.rel_diff(res, md.residual(x, rhs)))
            o.set(O.TNEW, l, x)
            o.copy_to_tnn(l)
            o.smoother(l)
            swept = md.sweep(x, rhs, solver)
            worst["sweep"] = max(worst["sweep"], F.rel_diff(o.get(O.TNN), swept))
            moved = min(moved, float(np.abs(swept - x).max()))
        share = min(share, float(np.abs(md.face_part(x)).max() / np.abs(md.apply(x)).max()))
        if (md.interior & ~md.inner).any():
            swapped = min(swapped, F.rel_diff(res, md.residual(x, rhs, swap_outer=True)))
    print(f"{mesh} {pset}: " + " ".join(f"{k}={v:.2e}" for k, v in worst.items()) +
          f" face share>={share:.2f} moved>={moved:.2f} swapped>={swapped:.2e}")
    for k, v in worst.items():
        assert v <= BOUND, (k, v)
    assert moved > 0.1
    if pset == "P2":
        assert share >= 0.25
        assert swapped > 1e-3


def test_model_source_is_the_cascade_not_the_mass_product():
    """the trap the module docstring names: M f is far from s' (12 % of the RHS at dt = 0.05)"""
    md = model_of("untitled8.msh", S, 1, "P2")
    f = -(2 * md.k) * np.sin(md.P[..., 0] + md.P[..., 1])
    Mf = np.einsum("usij,usj->usi", md.M, f).transpose(2, 1, 0)
    assert F.rel_diff(Mf, md.source_level1()) > 0.05


def test_variants_reach_every_interface_triple_and_boundary_pattern():
    """the three committed variants together show all 18 (face, fNeig, Dir) triples, four of which no fixture
    shows; variants, fixtures and one_tri together show all 8 boundary patterns of an un_ele"""
    all_meshes = sorted(f for f in os.listdir(goldens.MESHES) if f.endswith(".msh"))
    of_variants = set().union(*(V.interface_triples(mesh_of(n)) for n in VARIANTS))
    of_fixtures = set().union(*(V.interface_triples(O.read_msh(path_of(n))) for n in all_meshes if n not in VARIANTS))
    assert of_variants == V.ALL_TRIPLES and len(V.ALL_TRIPLES) == 18
    assert V.ALL_TRIPLES - of_fixtures == {(1, 1, 1), (1, 2, 0), (2, 1, 0), (3, 3, 1)}
    patterns = set().union(*(V.boundary_patterns(mesh_of(n)) for n in FIXTURES + VARIANTS))
    assert patterns == V.ALL_PATTERNS and len(V.ALL_PATTERNS) == 8


def test_committed_variants_are_reproducible(tmp_path):
    """tests/meshes/*_rn.msh are what renumber writes from the fixtures at the recorded seeds, with the same
    triangles: every un_ele of the fixture is one of the variant with the same vertices"""
    for name, (src, seed) in V.VARIANTS.items():
        out = str(tmp_path / name)
        V.renumber(path_of(src), out, seed)
        with open(out) as f, open(path_of(name)) as g:
            assert f.read() == g.read(), name
        a, b = mesh_of(src), mesh_of(name)
        assert a.U == b.U
        tri = lambda m: sorted(sorted(map(tuple, t)) for t in m.X.reshape(m.U, 3, 2).tolist())  # noqa: E731
        assert tri(a) == tri(b)
        assert sorted(a.region.tolist()) == sorted(b.region.tolist())


def test_renumber_switches(tmp_path):
    src = path_of("irregular.msh")
    same = str(tmp_path / "same.msh")
    V.renumber(src, same, 5, rotate=False, flip=False, permute=False)
    a, b = O.read_msh(src), O.read_msh(same)
    for k in ("X", "region", "neig", "fneig", "dir"):
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k))
    rot = str(tmp_path / "rot.msh")
    V.renumber(src, rot, 5, flip=False, permute=False)
    c = O.read_msh(rot)
    np.testing.assert_array_equal(c.region, a.region)   # the order is kept, the orientation too
    Xa, Xc = a.X.reshape(-1, 3, 2), c.X.reshape(-1, 3, 2)
    assert any((Xa[u] != Xc[u]).any() for u in range(a.U))
    for u in range(a.U):
        assert any((np.roll(Xa[u], s, axis=0) == Xc[u]).all() for s in range(3))


# ---------------------------------------------------------------- the whole cycle commutes with renumbering
def coordinate_source(P, area, dt):
    """a level-1 source term defined by coordinates alone (the built-in one is a cascade over the local node
    order, which does not commute with renumbering): area / dt * cos(2x - 3y), the scale of the RHS's other
    part M told / dt for a told of order 1, so that both parts count"""
    return (area[..., None] / dt * np.cos(2 * P[..., 0] - 3 * P[..., 1])).astype(np.float64).transpose(2, 1, 0)


PAIRS = [("untitled8.msh", "untitled8_rn.msh", 3, 3), ("irregular.msh", "irregular_rn.msh", 3, 3),
         ("test_sn2.msh", "test_sn2_rn.msh", 3, 2)]


@pytest.mark.parametrize("solver", [1, 3])
@pytest.mark.parametrize("cycle", [0, 1])
@pytest.mark.parametrize("op", [0, 1])
@pytest.mark.parametrize("a,b,n_split,levels", PAIRS, ids=[p[0].split(".")[0] for p in PAIRS])
def test_cycle_commutes_with_renumbering(a, b, n_split, levels, op, cycle, solver):
    """Oracle only: P1, 2 steps of 2 cycles on a fixture and on its renumbered variant from the same
    coordinate-defined source; tnew of every level and res_L1, matched by coordinates, within 1e-10 of the
    field's maximum. This pins the restrictor, the prolongator / interpolation and element_conversion
    independently of any numbering. Measured maxima over the eight (op, cycle, solver): untitled8 2.9e-14,
    irregular 1.8e-12 (op 0, cycle 1), test_sn2 1.1e-13."""
    states, maps = [], []
    for name in (a, b):
        m = mesh_of(name)
        o = O.Oracle(m, n_split, levels, solver=solver, op=op, ntime=2, n_multigrid=2, **SETS["P1"])
        md1 = model_of(name, n_split, 1, "P1")
        o.set_source(coordinate_source(md1.P, md1.area, md1.dt))
        drive(o, cycle, True)
        states.append(o.state())
        maps.append([model_of(name, n_split, l, "P1").P for l in range(1, levels + 1)])
    worst = 0.0
    for key in [f"tnew_L{l}" for l in range(1, levels + 1)] + ["res_L1"]:
        l = int(key[-1])
        idx = F.coordinate_map(maps[0][l - 1], maps[1][l - 1])
        ref = states[0][key]
        assert np.isfinite(ref).all() and np.abs(ref).max() > 0
        e = goldens.rel_err(F.renumbered(states[1][key], idx), ref)
        worst = max(worst, e)
        assert e <= CYCLE_BOUND, (key, e)
    print(f"{a} op={op} cycle={cycle} solver={solver}: worst {worst:.2e}")
