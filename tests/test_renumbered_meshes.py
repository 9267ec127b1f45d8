"""The HIP path on renumbered meshes: against the coordinate model, the oracle and the single domain.

Everything that crosses an un_ele face branches on (face, fNeig, Dir): the device halo tables, k_face_pp's
in-launch ghost words, the chain hand-offs, the exchange plans of pamg_plan.cpp. The fixtures show 14 of
the 18 triples an interior face can have; (1,1,1), (1,2,0), (2,1,0) and (3,3,1) occur only in the
renumbered variants of tests/mesh_variants.py (three committed under tests/meshes, the 900_ele and
untitled2048 ones written per session). The CPU side of the same matrix is tests/test_face_model.py.

  1. pamg_get_residual and one pamg_smoother call against tests/face_model.py directly, not through
     the oracle: the operator assembled from coordinates is what the kernels must compute.
  2. Every form of the cycle bit for bit the oracle on variants (tests/test_parameters.py's pattern: the
     oracle takes the device's source term; a configuration counts only if the oracle's final state is
     finite with max|tnew| <= 10).
  3. Partitions through the multi-rank exchange path bit for bit the single domain.
"""
import os

import numpy as np
import pytest

import face_model as F
import goldens
import mesh_variants as V
import oracle_lib as O
from test_parameters import P1, SETS, assert_states_equal, drive, full_state, gpu_solver, oracle_state

pytestmark = pytest.mark.gpu

MISSING_IN_FIXTURES = {(1, 1, 1), (1, 2, 0), (2, 1, 0), (3, 3, 1)}
BOUND = 1e-12   # of the model field's maximum (tests/test_face_model.py: the oracle is within 4.2e-14)


def path_of(mesh):
    return os.path.join(goldens.MESHES, mesh)


@pytest.fixture(scope="module")
def tmp_variants(tmp_path_factory):
    """renumbered 900_ele and untitled2048, each showing at least the four triples no fixture has"""
    d = tmp_path_factory.mktemp("variants")
    out = {}
    for src, seed in (("900_ele.msh", 1), ("untitled2048.msh", 1)):
        p = str(d / src.replace(".msh", "_rn.msh"))
        V.renumber(path_of(src), p, seed)
        assert MISSING_IN_FIXTURES <= V.interface_triples(O.read_msh(p)), src
        out[os.path.basename(p)] = p
    return out


def resolve(mesh, tmp_variants):
    return tmp_variants.get(mesh) or path_of(mesh)


# ---------------------------------------------------------------- 1. HIP against the model
_MODELS = {}


def model_of(mesh, n_split, level):
    key = (mesh, n_split, level)
    if key not in _MODELS:
        p = SETS["P2"]
        _MODELS[key] = F.FaceModel(O.read_msh(path_of(mesh)).X, n_split, level, p["dt"], p["k"], p["omega"])
    return _MODELS[key]


@pytest.mark.parametrize("arith", [0, 1])
@pytest.mark.parametrize("solver", [1, 3])
@pytest.mark.parametrize("mesh", sorted(V.VARIANTS) + ["irregular.msh", "test_sn2.msh"])
def test_hip_operator_is_the_coordinate_model(mesh, solver, arith):
    """P2 (the face terms are at least 0.4 of max |A x|), from random tnew / told / RHS: level 1's RHS, the residual
    of pamg_get_residual and the iterate after one pamg_smoother call with n_smooth = 1, on every level of
    (mesh, S 3, L 3) and on level 1 of (mesh, S 4, L 3) -- 256 sub-elements per un_ele, the tiled kernels.
    Level 1's s' is read back from the device and given to the model. Within 1e-12 of the model field's
    maximum, both arithmetics (arith = 1 is within about 1e-15 of arith = 0). Measured on an MI355X: at most
    1.3e-14 (irregular_rn, S 4, level 1, the residual), RHS at most 3.1e-16."""
    import pamg
    rng = np.random.default_rng(20251020)
    worst = 0.0
    for n_split, levels in ((3, (1, 2, 3)), (4, (1,))):
        g = gpu_solver((mesh, n_split, 3), "P2", n_smooth=1, solver=solver, arith=arith, op=1)
        source = g.get(pamg.SOURCE, 1)
        for l in levels:
            md = model_of(mesh, n_split, l)
            x, xo, b = (rng.uniform(-1, 1, (3, md.nsub, g.U)) for _ in range(3))
            rhs, e_rhs = b, 0.0
            if l == 1:
                # the device assembles level 1's RHS = M told / dt + s' once per step, in pamg_begin_timestep
                # (told := tnew first), where the reference and the oracle rebuild it at every visit
                g.set(pamg.TNEW, 1, xo)
                g.begin_timestep()
                rhs = md.rhs_level1(xo, source)
                e_rhs = F.rel_diff(g.get(pamg.RHS, 1), rhs)
                g.set(pamg.TNEW, 1, x)
            else:
                for what, v in ((pamg.TNEW, x), (pamg.TOLD, xo), (pamg.RHS, b)):
                    g.set(what, l, v)
            g.get_residual(l)
            e_res = F.rel_diff(g.get(pamg.RESIDUAL, l), md.residual(x, rhs))
            g.set(pamg.TNEW, l, x)
            g.copy_to_tnn(l)
            g.smoother(l, 1)
            swept = md.sweep(x, rhs, solver)
            assert np.abs(swept - x).max() > 0.1
            e_sweep = F.rel_diff(g.get(pamg.TNEW_NONLIN), swept)
            print(f"{mesh} S{n_split} level {l} solver {solver} arith {arith}: RHS {e_rhs:.2e} residual {e_res:.2e} "
                  f"sweep {e_sweep:.2e}")
            worst = max(worst, e_rhs, e_res, e_sweep)
            assert e_rhs <= BOUND, (n_split, l, e_rhs)
            assert e_res <= BOUND, (n_split, l, e_res)
            assert e_sweep <= BOUND, (n_split, l, e_sweep)
        g.close()
    print(f"{mesh} solver {solver} arith {arith}: worst {worst:.2e}")


# ---------------------------------------------------------------- 2. bitwise the oracle
# k_face_pp at 256 and 1,024 sub-elements per un_ele with its ghost words; the coarsest level as the per-wave
# chain; four levels; two meshes large enough for every triple at once
FACE_SHAPES = [("irregular_rn.msh", 4, 3), ("irregular_rn.msh", 5, 3), ("untitled8_rn.msh", 5, 3),
               ("test_sn2_rn.msh", 4, 4), ("900_ele_rn.msh", 3, 3), ("untitled2048_rn.msh", 4, 3)]


def shape_id(shape):
    return "{}-S{}-L{}".format(shape[0].split(".")[0], shape[1], shape[2])


@pytest.mark.parametrize("pset", ["default", "P1"])
@pytest.mark.parametrize("solver", [1, 3])
@pytest.mark.parametrize("cycle", [0, 1])
@pytest.mark.parametrize("shape", FACE_SHAPES, ids=shape_id)
def test_face_operator_on_variants_is_bitwise_the_oracle(shape, cycle, solver, pset, tmp_variants):
    """op = 1, the default form (the fused cycle: k_face_pp passes, the coarsest level's chain) and the
    per-step kernels (fused = 0): every field of every level, t_overlap and t_overlap_old equal the oracle's"""
    shape = (resolve(shape[0], tmp_variants),) + shape[1:]
    for fused in (3, 0):
        g = gpu_solver(shape, pset, solver=solver, cycle=cycle, op=1, fused=fused)
        ref = oracle_state(shape, pset, g, cycle=cycle, solver=solver, op=1)
        drive(g)
        assert_states_equal(full_state(g), ref, f"fused={fused}")
        g.close()


@pytest.mark.parametrize("cycle", [0, 1])
def test_face_operator_on_a_variant_without_the_chain(cycle, monkeypatch):
    """PAMG_FACE_CHAIN=0: (untitled8_rn, 5, 3)'s coarsest level with one launch per sweep instead of the chain"""
    monkeypatch.setenv("PAMG_FACE_CHAIN", "0")
    shape = ("untitled8_rn.msh", 5, 3)
    g = gpu_solver(shape, "P1", cycle=cycle, op=1)
    ref = oracle_state(shape, "P1", g, cycle=cycle, solver=3, op=1)
    drive(g)
    assert_states_equal(full_state(g), ref)
    g.close()


@pytest.mark.parametrize("arith", [0, 1])
@pytest.mark.parametrize("pset", ["default", "P1"])
@pytest.mark.parametrize("shape", [("untitled8_rn.msh", 5, 3), ("irregular_rn.msh", 4, 2)], ids=shape_id)
def test_every_fused_form_on_variants_is_bitwise_the_oracle(shape, pset, arith):
    """op = 0: fused 0, 1, 2 and 3 (the resident call; k_vc_resb<5,3> on (untitled8_rn, 5, 3)); here the halo
    arrays are the only place the triples show, so t_overlap and t_overlap_old are part of the comparison"""
    for fused in (0, 1, 2, 3):
        g = gpu_solver(shape, pset, arith=arith, fused=fused)
        ref = oracle_state(shape, pset, g, arith=arith)
        assert {"t_overlap", "t_overlap_old"} <= set(ref) and np.abs(ref["t_overlap"]).max() > 0
        drive(g)
        assert_states_equal(full_state(g), ref, f"fused={fused}")
        g.close()


# ---------------------------------------------------------------- 3. partitions
PART_SHAPES = {"900_ele_rn.msh": (3, 3), "untitled2048_rn.msh": (3, 3), "irregular_rn.msh": (4, 3)}
# op, cycle, PAMG_FACE_AGG: op = 0 as the resident call; op = 1 with the coarsest level agglomerated and partitioned
PART_FORMS = [(0, 0, None), (1, 0, "1"), (1, 1, "1"), (1, 0, "0"), (1, 1, "0")]
_SINGLE = {}


def single_domain(mesh, path, op, cycle):
    """the single domain's final state, computed once per (mesh, op, cycle) and shared read-only"""
    import pamg
    key = (mesh, op, cycle)
    if key not in _SINGLE:
        S, L = PART_SHAPES[mesh]
        full = pamg.SemiImplicitIterative(pamg.Mesh.read(path), S, L, op=op, cycle=cycle, **P1)
        drive(full)
        st = full_state(full)
        full.close()
        assert all(np.isfinite(v).all() for v in st.values())
        for v in st.values():
            v.setflags(write=False)
        _SINGLE[key] = st
    return _SINGLE[key]


@pytest.mark.parametrize("op,cycle,agg", PART_FORMS, ids=["op0", "op1-c0-agg", "op1-c1-agg", "op1-c0-part", "op1-c1-part"])
@pytest.mark.parametrize("kind", ["strip", "block"])
@pytest.mark.parametrize("nranks", [2, 3, 4])
@pytest.mark.parametrize("mesh", sorted(PART_SHAPES))
def test_partitions_of_variants_match_single_domain(mesh, nranks, kind, op, cycle, agg, tmp_variants, monkeypatch):
    """local_group (the multi-rank exchange path with device copies, tests/test_multirank.py) at P1, 2 steps of
    2 cycles: every field of every level and the halo arrays on each rank's un_eles equal the single domain's"""
    import pamg
    from pamg.solver import local_group, run_ranks
    if agg is not None:
        monkeypatch.setenv("PAMG_FACE_AGG", agg)
    path = resolve(mesh, tmp_variants)
    S, L = PART_SHAPES[mesh]
    ref = single_domain(mesh, path, op, cycle)
    m = pamg.Mesh.read(path)
    owner = m.x_strip_owner(nranks) if kind == "strip" else m.block_owner(nranks)
    parts = [pamg.SemiImplicitIterative(m, S, L, op=op, cycle=cycle, comm=(nranks, r, None, owner), **P1)
             for r in range(nranks)]
    local_group(parts)
    if op == 0:
        for p in parts:
            p.timing_enable(1 << 12)   # PAMG_K_VCYCLE_RES
            p.timing_reset()
    run_ranks(parts, drive)
    for r, p in enumerate(parts):
        own = np.flatnonzero(owner == r)
        assert p.U == len(own)
        for k, v in full_state(p).items():
            np.testing.assert_array_equal(v, ref[k][:, :, own], err_msg=f"rank {r} {k}")
        if op == 0:
            assert p.timing()["vcycle_res"]["issued"] > 0
        p.close()
