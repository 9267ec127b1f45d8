"""The level transfers and the corrected V-cycle (cycle = 1) against a model assembled from coordinates.

The corrected cycle and the face-coupled operator define their own arithmetic: no reference output exists
for them, and every HIP form is held bit for bit to oracle/pamg_oracle.c. tests/face_model.py pins the
operator, level 1's right-hand side and one sweep to coordinates, one level at a time. This module pins what
joins the levels and what the cycle is made of:

  - the restrictor and the P1 interpolation, which the oracle takes from element_conversion and hard-coded
    child / node tables and the HIP side restates in k_restrict_tile, k_restrict_residual, k_prolong_tile,
    k_interp_add, the resident k_vc_corr and the face passes. tests/cycle_model.py finds parents, corner
    children and interpolation weights by geometry (centroid in triangle, barycentric coordinates);
  - the composition of the corrected cycle: the fresh residual with the b - A x sign, coarse levels started
    from zero, the correction added before the post-smoothing, n_coarse calls on the coarsest level;
  - the block-diagonal operator (op = 0) inside a cycle and the direct coarse solve (coarse_solver = 1).

CPU tests hold the oracle to the model, GPU tests hold the HIP path to the model directly (not through the
oracle). Every distance is the error figure of cycle_model.cycle_diffs (tnew-like fields against max |model
tnew_L1|; RHS and residuals against the largest |value| of the model's RHS and residual fields of that
cycle), and every bound is BOUND = 1e-12 of it, a hundredth of the project's 1e-10 bar; the transfers alone
are held to 1e-14 of the model field's maximum.
"""
import numpy as np
import pytest

import cycle_model as CM
import face_model as F
import oracle_lib as O
from test_face_model import FIXTURES, VARIANTS, mesh_of, model_of, path_of
from test_parameters import SETS

BOUND = 1e-12            # the cycle, in cycle_diffs' figure
TRANSFER_BOUND = 1e-14   # a transfer alone, of the model field's maximum
SEED = 20251021

_TRANSFERS = {}


def transfers_of(mesh, n_split, levels):
    """{l: TransferModel} for l = 1 .. levels - 1, built once per (mesh, n_split, l) and shared read-only"""
    out = {}
    for l in range(1, levels):
        key = (mesh, n_split, l)
        if key not in _TRANSFERS:
            _TRANSFERS[key] = CM.TransferModel(mesh_of(mesh).X, n_split, l)
        out[l] = _TRANSFERS[key]
    return out


def models_of(mesh, n_split, levels, pset):
    return {l: model_of(mesh, n_split, l, pset) for l in range(1, levels + 1)}


def n_smooth_of(n_split):
    return 4 if n_split >= 5 else 2


def random_start(mesh, n_split):
    return np.random.default_rng(SEED).uniform(-1, 1, (3, 4 ** n_split, mesh_of(mesh).U))


def full_mantissa(rng, shape):
    """random values in (-1, 1) whose last mantissa bits are in use. rng.uniform(-1, 1) alone lies on a grid of
    2^-52, on which the midpoints 0.5 a + 0.5 b are exact in fp64: the interpolation would then show a distance
    of exactly 0 and the rounding it really has would go unmeasured."""
    return rng.uniform(-1, 1, shape) * rng.uniform(0.5, 1, shape)


def model_looks(mesh, n_split, levels, pset, op, solver, coarse_solver=0, schedule=((1, 1), (1, 1)), source=None,
                transfers=None):
    """The model's run from random_start: one time step per entry of `schedule`, one call of c cycles per
    number c in it. Level 1's RHS is rebuilt at every step from the model's own iterate (told := tnew).
    Returns the (x, b, res) of corrected_cycle after the last cycle of every call, in order."""
    mds = models_of(mesh, n_split, levels, pset)
    trs = transfers_of(mesh, n_split, levels) if transfers is None else transfers
    p = SETS[pset]
    x, looks = random_start(mesh, n_split), []
    for step in schedule:
        rhs1 = mds[1].rhs_level1(x, source)
        for cycles in step:
            for _ in range(cycles):
                look = CM.corrected_cycle(mds, trs, x, rhs1, n_smooth_of(n_split), p["n_coarse"], solver, op,
                                          coarse_solver)
                x = look[0][1]
            looks.append(look)
    return looks


def oracle_against(looks, mesh, n_split, levels, pset, op, solver, arith, coarse_solver=0):
    """orc_vcycle_corrected from random_start, two steps of two cycles, compared with the model's looks after
    every cycle. Returns the worst figure per kind and the oracle's peak |tnew| over the levels at the end."""
    p = SETS[pset]
    o = O.Oracle(mesh_of(mesh), n_split, levels, n_smooth=n_smooth_of(n_split), solver=solver, op=op, arith=arith,
                 coarse_solver=coarse_solver, **p)
    o.set(O.TNEW, 1, random_start(mesh, n_split))
    worst, it = dict(tnew=0.0, RHS=0.0, res=0.0), iter(looks)
    for _ in range(2):
        o.begin_timestep()
        for _ in range(2):
            o.vcycle_corrected()
            for k, v in CM.cycle_diffs(o.state(), *next(it)).items():
                worst[k] = max(worst[k], v)
    st = o.state()
    assert all(np.isfinite(v).all() for v in st.values()), "inadmissible: not finite"
    peak = max(float(np.abs(st[f"tnew_L{l}"]).max()) for l in range(1, levels + 1))
    return worst, peak


def correction_size(looks, transfers):
    """max |interpolate(x_2)| / max |x_1| of the first cycle: what the coarse levels contribute"""
    x = looks[0][0]
    return float(np.abs(transfers[1].interpolate(x[2])).max() / np.abs(x[1]).max())


# ---------------------------------------------------------------- a. the transfers alone
@pytest.mark.parametrize("mesh", FIXTURES + VARIANTS)
def test_oracle_transfers_are_the_coordinate_model(mesh):
    """orc_restrictor from a random residual, and orc_prolongator onto a zero fine tnew (with a zero fine
    field the reference's cascade is the interpolation), on both level pairs of (mesh, S 3, L 3): within 1e-14
    of the model field's maximum. Measured maxima over the nine meshes: restrictor 1.7e-16, prolongator
    7.4e-17 (the restrictor's two additions and division, the prolongator's one rounding of a midpoint). The
    inputs come from full_mantissa: on rng.uniform's own grid the prolongator's distance is exactly 0."""
    S, L = 3, 3
    m, trs = mesh_of(mesh), transfers_of(mesh, S, L)
    o = O.Oracle(m, S, L)
    rng = np.random.default_rng(SEED)
    for l in range(1, L):
        t = trs[l]
        r, y = full_mantissa(rng, (3, t.nf, m.U)), full_mantissa(rng, (3, t.nc, m.U))
        o.set(O.RES, l, r)
        o.restrictor(l)
        e_r = F.rel_diff(o.get(O.RHS, l + 1), t.restrict(r))
        o.set(O.TNEW, l, np.zeros_like(r))
        o.set(O.TNEW, l + 1, y)
        o.prolongator(l)
        e_p = F.rel_diff(o.get(O.TNEW, l), t.interpolate(y))
        print(f"{mesh} level {l}: restrictor {e_r:.2e} prolongator {e_p:.2e}")
        assert e_r <= TRANSFER_BOUND, (l, e_r)
        assert e_p <= TRANSFER_BOUND, (l, e_p)


# ---------------------------------------------------------------- b. the cycle
SHAPES = ([(m, 3, 3) for m in FIXTURES + VARIANTS] +
          [("untitled8_rn.msh", 5, 3), ("irregular_rn.msh", 4, 3), ("test_sn2_rn.msh", 4, 4), ("untitled8.msh", 2, 2),
           ("untitled8.msh", 5, 5)])
# (parameter set, op, solver, coarse_solver)
FORMS = ([(p, op, solver, 0) for p in ("default", "P1", "P3", "P4") for op in (0, 1) for solver in (1, 3)] +
         [("P2", 1, 3, 0)] + [(p, 0, 3, 1) for p in ("default", "P1", "P3", "P4")])


def shape_id(shape):
    return "{}-S{}-L{}".format(shape[0].split(".")[0], shape[1], shape[2])


def form_id(form):
    return "{}-op{}-solver{}".format(*form[:3]) + ("-direct" if form[3] else "")


@pytest.mark.parametrize("form", FORMS, ids=form_id)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_oracle_corrected_cycle_is_the_coordinate_model(shape, form):
    """orc_vcycle_corrected from a seeded random level-1 tnew, two time steps of two cycles, compared after
    every cycle, arith 0 and 1 (one model run serves both): tnew and RHS of every level, res_l for 1 < l < L and
    the final res_1 within 1e-12 in cycle_diffs' figure. n_smooth is 2, and 4 at n_split 5.

    Left out, because the problem and not the model is at fault there:
      - P2 with op = 0: its blocks are near-singular (a pure-Neumann stiffness plus a small mass term), so the
        comparison measures their conditioning: 4.7e-11 at S 5, 5e-13 at S 3.
      - P2 with solver 1: inadmissible on test_sn2, test_sn2_rn and (irregular_rn, 4, 3), where max |tnew|
        reaches 11 to 15.
    Every case listed is admissible on the oracle (finite, max |tnew| <= 10 on every level), asserted below.

    Measured maxima over the forms and both arithmetics, per shape:
      2_unele_test 1.4e-14   900_ele      6.1e-14   irregular    1.7e-14   one_tri      4.2e-15   test_sn2 1.3e-14
      untitled8    1.0e-14   untitled8_rn 1.3e-14   irregular_rn 1.4e-14   test_sn2_rn  9.0e-15
      (untitled8_rn, 5, 3) 4.2e-14   (irregular_rn, 4, 3) 1.6e-14   (test_sn2_rn, 4, 4) 1.3e-14
      (untitled8, 2, 2) 8.3e-15      (untitled8, 5, 5) 6.6e-14
    and per parameter set (op 0 / op 0 with the direct solve / op 1): default 3.6e-15 / 4.2e-15 / 2.8e-14, P1 3.7e-14 /
    4.1e-14 / 1.7e-14, P3 5.3e-15 / 5.2e-15 / 6.6e-14, P4 4.3e-14 / 4.1e-14 / 1.7e-14, P2 op 1 6.1e-14. The worst are
    6.6e-14 on (untitled8, 5, 5) at P3, op = 1, solver 1 and 6.1e-14 on (900_ele, 3, 3) at P2 (its un_eles are small
    against their distance from the origin: the oracle's fp64 coordinates carry the largest relative error). The
    bound keeps 15 times margin; the largest final max |tnew| is 1.1."""
    (mesh, S, L), (pset, op, solver, cs) = shape, form
    looks = model_looks(mesh, S, L, pset, op, solver, cs)
    for arith in (0, 1):
        worst, peak = oracle_against(looks, mesh, S, L, pset, op, solver, arith, cs)
        print(f"{shape_id(shape)} {form_id(form)} arith {arith}: " + " ".join(f"{k}={v:.2e}" for k, v in worst.items()) +
              f" peak {peak:.2f}")
        assert peak <= 10.0, ("inadmissible", peak)
        for k, v in worst.items():
            assert v <= BOUND, (arith, k, v)


# ---------------------------------------------------------------- c. guards
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_coarse_correction_is_a_large_part_of_the_iterate(shape):
    """P2, op = 1, solver 3: the first cycle's correction max |interpolate(x_2)| / max |x_1| is at least 0.1
    (measured: at least 0.228, on 2_unele_test; 0.26 to 0.73 elsewhere), so a cycle that dropped or misplaced it could not pass"""
    mesh, S, L = shape
    looks = model_looks(mesh, S, L, "P2", 1, 3, schedule=((1,),))
    c = correction_size(looks, transfers_of(mesh, S, L))
    print(f"{shape_id(shape)}: correction {c:.3f}")
    assert c >= 0.1


MUTANTS = ("corners_rotated", "injection", "nodes_swapped")


@pytest.mark.parametrize("op", [0, 1])
@pytest.mark.parametrize("kind", MUTANTS)
def test_wrong_transfers_are_far_from_the_oracle(kind, op):
    """(untitled8_rn, 3, 3) at P1, solver 3: the model with the corner children rotated by one vertex, with
    the interpolation replaced by injection of the parent's own node values, or with two coarse nodes
    swapped in the interpolation weights, is at least 1e-4 from the oracle (measured: at least 4.5e-2; the
    smallest single figure of a mutant is 1.7e-2, the RHS under injection at op = 0)"""
    mesh, S, L = "untitled8_rn.msh", 3, 3
    trs = {l: t.mutant(kind) for l, t in transfers_of(mesh, S, L).items()}
    looks = model_looks(mesh, S, L, "P1", op, 3, transfers=trs)
    worst, _ = oracle_against(looks, mesh, S, L, "P1", op, 3, 0)
    print(f"{kind} op {op}: " + " ".join(f"{k}={v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) >= 1e-4


@pytest.mark.parametrize("kind", MUTANTS)
def test_wrong_transfers_are_seen_by_the_transfer_test(kind):
    """the same mutants against orc_restrictor / orc_prolongator alone: the mutated transfer is of order 1 away"""
    mesh, S, L = "untitled8_rn.msh", 3, 3
    m = mesh_of(mesh)
    o = O.Oracle(m, S, L)
    rng = np.random.default_rng(SEED)
    for l, t in transfers_of(mesh, S, L).items():
        r, y = full_mantissa(rng, (3, t.nf, m.U)), full_mantissa(rng, (3, t.nc, m.U))
        o.set(O.RES, l, r)
        o.restrictor(l)
        o.set(O.TNEW, l, np.zeros_like(r))
        o.set(O.TNEW, l + 1, y)
        o.prolongator(l)
        mt = t.mutant(kind)
        e = max(F.rel_diff(o.get(O.RHS, l + 1), mt.restrict(r)), F.rel_diff(o.get(O.TNEW, l), mt.interpolate(y)))
        assert e >= 0.1, (l, e)


@pytest.mark.parametrize("solver", [1, 3])
@pytest.mark.parametrize("op", [0, 1])
@pytest.mark.parametrize("pset", ["default", "P1", "P2"])
def test_one_level_cycle_is_smoothing_only(pset, op, solver):
    """L = 1 on (one_tri, 1, 1): the cycle is n_smooth sweeps and the residual, and the model still matches"""
    looks = model_looks("one_tri.msh", 1, 1, pset, op, solver)
    for arith in (0, 1):
        worst, _ = oracle_against(looks, "one_tri.msh", 1, 1, pset, op, solver, arith)
        for k, v in worst.items():
            assert v <= BOUND, (arith, k, v)
    x0, md = random_start("one_tri.msh", 1), model_of("one_tri.msh", 1, 1, pset)
    b, x = md.rhs_level1(x0), x0
    for _ in range(n_smooth_of(1)):
        x = md.sweep(x, b, solver) if op == 1 else md.sweep0(x, b)
    assert np.array_equal(x, looks[0][0][1])


# ---------------------------------------------------------------- GPU: HIP against the model, directly
gpu = pytest.mark.gpu


def gpu_solver(mesh, n_split, levels, pset, **kw):
    import pamg
    return pamg.SemiImplicitIterative(pamg.Mesh.read(path_of(mesh)), n_split, levels, **SETS[pset], **kw)


@gpu
@pytest.mark.parametrize("op", [0, 1])
@pytest.mark.parametrize("mesh,n_split,pairs", [("untitled8_rn.msh", 3, (1, 2)), ("irregular_rn.msh", 5, (1, 2))],
                         ids=["untitled8_rn-S3", "irregular_rn-S5"])
def test_hip_transfers_are_the_coordinate_model(mesh, n_split, pairs, op):
    """pamg_restrictor(l) from a residual set on the device and pamg_prolongator(l) onto a zero fine tnew: every
    level pair of (untitled8_rn, 3, 3), and levels 1 and 2 of (irregular_rn, 5, 3) -- 1,024 and 256 sub-elements
    per un_ele, the tiled kernels and their LDS path -- with op 0 and 1, within 1e-14 of the model field's
    maximum. Measured on an MI355X: restrictor at most 1.5e-16, prolongator at most 6.0e-17, on both shapes."""
    import pamg
    L = 3
    g = gpu_solver(mesh, n_split, L, "P1", op=op)
    trs = transfers_of(mesh, n_split, L)
    rng = np.random.default_rng(SEED)
    for l in pairs:
        t = trs[l]
        r, y = full_mantissa(rng, (3, t.nf, g.U)), full_mantissa(rng, (3, t.nc, g.U))
        g.set(pamg.RESIDUAL, l, r)
        g.restrictor(l)
        e_r = F.rel_diff(g.get(pamg.RHS, l + 1), t.restrict(r))
        g.set(pamg.TNEW, l, np.zeros_like(r))
        g.set(pamg.TNEW, l + 1, y)
        g.prolongator(l)
        e_p = F.rel_diff(g.get(pamg.TNEW, l), t.interpolate(y))
        print(f"{mesh} S{n_split} op {op} level {l}: restrictor {e_r:.2e} prolongator {e_p:.2e}")
        assert e_r <= TRANSFER_BOUND, (l, e_r)
        assert e_p <= TRANSFER_BOUND, (l, e_p)
    g.close()


GPU_SHAPES = [("untitled8_rn.msh", 3, 3), ("irregular_rn.msh", 4, 3), ("test_sn2_rn.msh", 4, 4), ("untitled8.msh", 2, 2),
              ("untitled8_rn.msh", 5, 3)]
GPU_FORMS = ([(p, 0, solver, 0) for p in ("P1", "default", "P4") for solver in (1, 3)] + [("P1", 0, 3, 1)] +
             [(p, 1, solver, 0) for p in ("P1", "default") for solver in (1, 3)] + [("P2", 1, 3, 0)])
GPU_SCHEDULE = ((2,), (1, 1))
_SOURCES = {}


@gpu
@pytest.mark.parametrize("form", GPU_FORMS, ids=form_id)
@pytest.mark.parametrize("shape", GPU_SHAPES, ids=shape_id)
def test_hip_corrected_cycle_is_the_coordinate_model(shape, form):
    """The HIP path with cycle = 1 from a random tnew over two time steps -- pamg_vcycle(2) in the first,
    pamg_vcycle(1) twice in the second -- compared with the model after every call (the model runs two cycles
    where the call ran two): tnew and RHS of every level, res_l for 1 < l < L and the final res_1 within 1e-12.
    The model takes the device's source term s'. One model run serves every variant of a form: op = 0 runs
    arith 0 and 1 with fused 3 (the resident k_vc_corr, one launch per call, asserted; whole-un_ele tiles on
    (untitled8_rn, 5, 3), the bench n_split; with the direct coarse solve the call runs the per-step kernels)
    and fused 0 (the per-step kernels); op = 1 runs its default form (on (untitled8_rn, 5, 3) k_face_pp<1024, ..>
    with the restrictor and the interpolation folded into its passes) and fused 0. At P2 the correction-size
    guard is taken on the HIP state too: after one pamg_vcycle(1) from the same start, max |interpolate(tnew_2)|
    / max |tnew_1| of the device's fields is at least 0.1 (measured: 0.31 to 0.66).

    Measured on an MI355X, maxima over the forms and variants (op 0 / op 1): (untitled8_rn, 3, 3) 1.8e-15 / 1.3e-14,
    (irregular_rn, 4, 3) 9.6e-16 / 1.6e-14, (test_sn2_rn, 4, 4) 1.3e-15 / 1.3e-14, (untitled8, 2, 2) 9.4e-16 /
    8.3e-15, (untitled8_rn, 5, 3) 4.1e-14 / 2.0e-14. fused 3 and fused 0 give the same figures to every digit
    printed, arith = 1 is within 1.4e-14 of arith = 0. The bound keeps 24 times margin."""
    import pamg
    (mesh, S, L), (pset, op, solver, cs) = shape, form
    variants = [dict(arith=a, fused=f) for a in (0, 1) for f in (3, 0)] if op == 0 else [dict(fused=3), dict(fused=0)]
    common = dict(n_smooth=n_smooth_of(S), solver=solver, op=op, coarse_solver=cs, cycle=1)
    if pset == "P2":
        g = gpu_solver(mesh, S, L, pset, **common)
        g.set(pamg.TNEW, 1, random_start(mesh, S))
        g.begin_timestep()
        g.vcycle(1)
        c = float(np.abs(transfers_of(mesh, S, L)[1].interpolate(g.get(pamg.TNEW, 2))).max() /
                  np.abs(g.get(pamg.TNEW, 1)).max())
        g.close()
        print(f"{shape_id(shape)}: correction on the HIP state {c:.3f}")
        assert c >= 0.1
    looks = None
    for kw in variants:
        g = gpu_solver(mesh, S, L, pset, **common, **kw)
        source = g.get(pamg.SOURCE, 1)
        if looks is None:
            # s' depends on the mesh, n_split and k alone: every handle of this case must report the same
            looks = model_looks(mesh, S, L, pset, op, solver, cs, schedule=GPU_SCHEDULE, source=source)
            first_source = source
        np.testing.assert_array_equal(source, first_source, err_msg="source term")
        g.set(pamg.TNEW, 1, random_start(mesh, S))
        g.timing_enable(1 << 14)   # PAMG_K_VCYCLE_CORR
        g.timing_reset()
        worst, it = dict(tnew=0.0, RHS=0.0, res=0.0), iter(looks)
        for step in GPU_SCHEDULE:
            g.begin_timestep()
            for cycles in step:
                g.vcycle(cycles)
                for k, v in CM.cycle_diffs(g.state(), *next(it)).items():
                    worst[k] = max(worst[k], v)
        # the resident launch, one per call, where the docstring says so and nowhere else
        resident = op == 0 and cs == 0 and kw["fused"] == 3
        assert g.timing()["vcycle_corr"]["issued"] == (sum(len(step) for step in GPU_SCHEDULE) if resident else 0)
        g.close()
        print(f"{shape_id(shape)} {form_id(form)} {kw}: " + " ".join(f"{k}={v:.2e}" for k, v in worst.items()))
        for k, v in worst.items():
            assert v <= BOUND, (kw, k, v)
