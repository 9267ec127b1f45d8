"""Parity away from the reference's own dt, k, omga and sweep counts.

The reference hard-codes dt = CFL*dx = 1.25e-5, k = 1, omga = 0.8 and 15 smoother calls on the
coarsest level (transport_tri_semi.F90:133,136,140,351); pamg_params takes all four, and n_smooth,
as free inputs. k = 1 is the multiplicative identity (a factor dropped, doubled or misplaced is
invisible), 1/dt = 80,000 lets the mass term hide the diffusion rows, the fused and resident kernels
merge the coarsest level's 1 + n_coarse calls into one chain, and omega sits in tables built at setup.
The goldens with a `_p1` / `_p2` / `_nc0` / `_nc1` suffix (tests/make_golden.py) pin the oracle to the
reference at such values; here every GPU form is held to the oracle, bit for bit, at these sets:

    set   dt      k     omega  n_coarse
    P1    3.1e-4  0.37  0.65   3         every knob moved
    P2    0.05    3.0   0.8    15        the diffusion term dominates the mass term
    P3    7e-6    1.9   0.9    1         n_coarse = 1: the edge of the host's `n_coarse >= 1` branches
    P4    P1      P1    P1     0         the coarsest level is never swept

The oracle takes the device's source term s' (the one operation the two sides cannot share, the sine:
tests/test_contracted_oracle.py) and is computed once per configuration, shared by the forms compared
with it. A configuration is used only if the oracle's own final state is finite with max|tnew| <= 10
(the rule the goldens are admitted by): checked with the oracle for every case listed here; (irregular,
S 4, L 2) at P2 reaches 24 under the reference cycle and is not in the matrix.

n_smooth = 0 is refused by pamg_create and orc_create (include/pamg.h: the reference's sweep loop is
then empty and its get_RHS, called only inside it, never assembles level 1's right-hand side).
"""
import os

import numpy as np
import pytest

import goldens
import oracle_lib as O

gpu = pytest.mark.gpu

P1 = dict(dt=3.1e-4, k=0.37, omega=0.65, n_coarse=3)
P2 = dict(dt=0.05, k=3.0, omega=0.8, n_coarse=15)
P3 = dict(dt=7e-6, k=1.9, omega=0.9, n_coarse=1)
P4 = dict(P1, n_coarse=0)
SETS = {"P1": P1, "P2": P2, "P3": P3, "P4": P4, "default": dict(goldens.PHYSICS_DEFAULTS)}

U8_33, IRR_42, U8_53, U8_63, U8_55 = (("untitled8.msh", 3, 3), ("irregular.msh", 4, 2), ("untitled8.msh", 5, 3),
                                      ("untitled8.msh", 6, 3), ("untitled8.msh", 5, 5))
STEPS, CYCLES = 2, 2


def shape_id(shape):
    return "{}-S{}-L{}".format(shape[0].split(".")[0], shape[1], shape[2])


def path_of(mesh):
    return os.path.join(goldens.MESHES, mesh)


def gpu_solver(shape, pset, **kw):
    import pamg
    mesh, S, L = shape
    return pamg.SemiImplicitIterative(pamg.Mesh.read(path_of(mesh)), S, L, **SETS[pset], **kw)


def full_state(s):
    st = s.state()
    st["t_overlap"], st["t_overlap_old"] = s.overlap()
    return st


def drive(s, cycle=0, is_oracle=False):
    """STEPS time steps of CYCLES cycles: pamg_vcycle(CYCLES) per step, orc_vcycle[_corrected] per cycle"""
    for _ in range(STEPS):
        s.begin_timestep()
        if not is_oracle:
            s.vcycle(CYCLES)
            continue
        for _ in range(CYCLES):
            s.vcycle_corrected() if cycle else s.vcycle()


_REFERENCES = {}


def oracle_state(shape, pset, g, cycle=0, how="cycles", **kw):
    """The oracle's final state of this configuration from the device's source term, computed once and
    shared (read-only) by every form compared with it; the device's s' must be the same in each."""
    import pamg
    mesh, S, L = shape
    src = g.get(pamg.SOURCE, 1)
    key = (shape, pset, cycle, how, tuple(sorted(kw.items())))
    if key not in _REFERENCES:
        o = O.Oracle(O.read_msh(path_of(mesh)), S, L, ntime=STEPS, n_multigrid=CYCLES, **SETS[pset], **kw)
        o.set_source(src)
        o.run() if how == "run" else drive(o, cycle, True)
        st = full_state(o)
        peak = max(float(np.abs(st[f"tnew_L{l}"]).max()) for l in range(1, L + 1))
        assert all(np.isfinite(v).all() for v in st.values()) and peak <= 10.0, ("inadmissible", key, peak)
        for v in list(st.values()) + [src]:
            v.setflags(write=False)
        _REFERENCES[key] = (src, st)
    ref_src, st = _REFERENCES[key]
    np.testing.assert_array_equal(src, ref_src, err_msg="source term")
    return st


def assert_states_equal(got, ref, what=""):
    assert set(ref) <= set(got)
    for k, v in ref.items():
        np.testing.assert_array_equal(got[k], v, err_msg=f"{what} {k}")


# ---------------------------------------------------------------- CPU: the knobs are live, arith = 1's distance
def _oracle_tnew(shape, params, cycle, op):
    mesh, S, L = shape
    o = O.Oracle(O.read_msh(path_of(mesh)), S, L, op=op, **params)
    drive(o, cycle, True)
    return [o.get(O.TNEW, l) for l in range(1, L + 1)]


@pytest.mark.parametrize("op", [0, 1])
@pytest.mark.parametrize("cycle", [0, 1])
def test_every_knob_moves_the_oracle_state_at_p1(op, cycle):
    """Guard against a vacuous matrix: the oracle's final tnew at P1 differs by more than 1e-6 relative, on
    every level, from its tnew with any one of dt / k / omega / n_coarse put back to the default. The one
    exception is the reference's own: its cycle (cycle = 0) discards the coarse correction (SURVEY.md A3,
    the prolongator's result is overwritten, :550), so n_coarse reaches the coarsest level only; under the
    corrected cycle it reaches every level."""
    L = U8_33[2]
    base = _oracle_tnew(U8_33, P1, cycle, op)
    for key, default in goldens.PHYSICS_DEFAULTS.items():
        alt = _oracle_tnew(U8_33, dict(P1, **{key: default}), cycle, op)
        for l in range(1, L + 1):
            d = goldens.rel_err(alt[l - 1], base[l - 1])
            if key == "n_coarse" and cycle == 0 and l < L:
                assert d == 0.0, (key, l, d)
            else:
                assert d > 1e-6, (key, l, d)


@pytest.mark.parametrize("name", ["irregular_s3_l3_jacobi_p2", "u8_s3_l3_gs_p1"])
def test_contracted_arithmetic_distance_from_the_reference(name):
    """arith = 1 (fma rows of A_e = M/dt + Kd) against the reference's own output outside the mass-dominated
    default: every field of the final state within the project's bar, 1e-10 of the field's max. Measured
    maxima over the fields: 1.5e-15 at P2 (irregular_s3_l3_jacobi_p2, res_L1), 8.8e-15 at P1 (u8_s3_l3_gs_p1,
    res_L1); the level-1 solution is within 4e-16 in both."""
    meta, d = goldens.load(name)
    o = O.Oracle(O.read_msh(path_of(meta["mesh"])), meta["n_split"], meta["levels"], n_smooth=meta["n_smooth"],
                 solver=meta["solver"], ntime=meta["ntime"], n_multigrid=meta["n_multigrid"], arith=1,
                 **goldens.physics(meta))
    o.run()
    worst = 0.0
    for k, v in full_state(o).items():
        e = goldens.rel_err(v, d[k])
        worst = max(worst, e)
        assert e <= 1e-10, (k, e)
    print(f"{name}: max rel_err(oracle arith=1, reference) = {worst:.3e}")


def test_zero_sweeps_are_refused_by_the_oracle():
    m = O.read_msh(path_of("untitled8.msh"))
    with pytest.raises(ValueError):
        O.Oracle(m, 3, 3, n_smooth=0)
    O.Oracle(m, 3, 3, n_smooth=1, n_coarse=0)   # zero coarse calls are a valid cycle


@gpu
def test_zero_sweeps_are_refused_by_pamg_create():
    import pamg
    with pytest.raises(pamg.PamgError) as e:
        gpu_solver(U8_33, "P1", n_smooth=0)
    assert e.value.rc == -1   # PAMG_ERR_ARG
    gpu_solver(U8_33, "P1", n_smooth=1).close()


# ---------------------------------------------------------------- op = 0: per-step, fused, pipelined, resident
OP0 = ([(s, p) for s in (U8_33, IRR_42, U8_53, U8_63, U8_55) for p in ("P1", "P3", "P4")] +
       [(U8_33, "P2"), (U8_53, "P2")])


@gpu
@pytest.mark.parametrize("arith", [0, 1])
@pytest.mark.parametrize("shape,pset", OP0, ids=[f"{shape_id(s)}-{p}" for s, p in OP0])
def test_every_fused_form_is_bitwise_the_oracle(shape, pset, arith):
    """fused = 0 (one kernel per step), 1 and 2 (two launches per cycle), 3 (pipelined / resident: k_vc_res
    below n_split 5, the balanced-role k_vc_resb<5,3> on (untitled8, 5, 3), sub-un_ele tiles at n_split 6),
    both arithmetics: every field of every level and the halo arrays equal the oracle's, and so each other."""
    states = {}
    for fused in (0, 1, 2, 3):
        g = gpu_solver(shape, pset, arith=arith, fused=fused)
        ref = oracle_state(shape, pset, g, arith=arith)
        g.timing_enable(1 << 12)   # PAMG_K_VCYCLE_RES
        g.timing_reset()
        drive(g)
        # the pipelined call really ran as the resident launch, one per call; no other form uses it
        assert g.timing()["vcycle_res"]["issued"] == (STEPS if fused == 3 else 0)
        states[fused] = full_state(g)
        g.close()
        assert_states_equal(states[fused], ref, f"fused={fused}")
    assert_states_equal(states[3], states[0], "fused 3 vs 0")


@gpu
@pytest.mark.parametrize("arith", [0, 1])
@pytest.mark.parametrize("schedule", [1, 2, 3])
@pytest.mark.parametrize("pset", ["P1", "P4"])
def test_call_schedules_are_bitwise_the_oracle(pset, schedule, arith):
    """the pipelined call as one launch per cycle, two tile streams and the resident launch (P4 too: schedules
    1 and 2 run a call's first cycle through the two-launch coarse kernel, where n_coarse = 0 went wrong)"""
    g = gpu_solver(U8_53, pset, arith=arith, fused=3)
    g.set_call_schedule(schedule)
    ref = oracle_state(U8_53, pset, g, arith=arith)
    drive(g)
    assert_states_equal(full_state(g), ref)
    g.close()


@gpu
@pytest.mark.parametrize("arith", [0, 1])
@pytest.mark.parametrize("pset", ["P1", "P4"])
@pytest.mark.parametrize("shape", [U8_33, U8_53], ids=shape_id)
def test_pamg_run_is_orc_run(shape, pset, arith):
    """pamg_run (the time loop in one resident launch) against orc_run"""
    g = gpu_solver(shape, pset, arith=arith)
    ref = oracle_state(shape, pset, g, how="run", arith=arith)
    g.run(STEPS, CYCLES)
    assert_states_equal(full_state(g), ref)
    g.close()


# ---------------------------------------------------------------- the corrected cycle, the direct coarse solve
@gpu
@pytest.mark.parametrize("arith", [0, 1])
@pytest.mark.parametrize("pset", ["P1", "P3", "P4"])
@pytest.mark.parametrize("solver", [1, 3])
@pytest.mark.parametrize("shape", [U8_33, U8_53], ids=shape_id)
def test_corrected_cycle_is_bitwise_the_oracle(shape, solver, pset, arith):
    """cycle = 1: the resident call (k_vc_corr) and the per-step path (fused = 0) equal orc_vcycle_corrected"""
    for fused in (3, 0):
        g = gpu_solver(shape, pset, solver=solver, arith=arith, cycle=1, fused=fused)
        ref = oracle_state(shape, pset, g, cycle=1, solver=solver, arith=arith)
        g.timing_enable(1 << 14)   # PAMG_K_VCYCLE_CORR
        g.timing_reset()
        drive(g)
        assert g.timing()["vcycle_corr"]["issued"] == (STEPS if fused == 3 else 0)
        assert_states_equal(full_state(g), ref, f"fused={fused}")
        g.close()


@gpu
@pytest.mark.parametrize("cycle", [0, 1])
@pytest.mark.parametrize("pset", ["P1", "P2"])
@pytest.mark.parametrize("shape", [U8_33, ("900_ele.msh", 2, 2)], ids=shape_id)
def test_direct_coarse_solve_is_bitwise_the_oracle(shape, pset, cycle):
    """coarse_solver = 1 inverts A_e = (1/dt) M + Kd itself: k and dt enter the matrix directly"""
    g = gpu_solver(shape, pset, coarse_solver=1, cycle=cycle)
    ref = oracle_state(shape, pset, g, cycle=cycle, coarse_solver=1)
    drive(g)
    assert_states_equal(full_state(g), ref)
    g.close()


# ---------------------------------------------------------------- op = 1: the face-coupled operator
U8_33F, IRR_43F, U8_53F = U8_33, ("irregular.msh", 4, 3), U8_53


@gpu
@pytest.mark.parametrize("pset", ["P1", "P2", "P4"])
@pytest.mark.parametrize("cycle", [0, 1])
@pytest.mark.parametrize("solver", [1, 3])
@pytest.mark.parametrize("shape", [U8_33F, IRR_43F, U8_53F], ids=shape_id)
def test_face_operator_is_bitwise_the_oracle(shape, solver, cycle, pset):
    """k enters the face weights w_f = k / dx |e| / 6 and the diagonal, omega the per-pattern omega/D tables;
    on (untitled8, 5, 3) level 3 runs as the persistent chain in its per-wave form and level 1 as
    k_face_pp<1024,512>. Every (shape, solver, cycle, set) here is admissible on the oracle."""
    g = gpu_solver(shape, pset, solver=solver, cycle=cycle, op=1)
    ref = oracle_state(shape, pset, g, cycle=cycle, solver=solver, op=1)
    drive(g)
    assert_states_equal(full_state(g), ref)
    g.close()


@gpu
@pytest.mark.parametrize("form", ["chain_off", "per_step"])
def test_face_operator_other_forms_equal_the_default_form(form, monkeypatch):
    """P1 on (untitled8, 5, 3): the coarsest level without the persistent chain (PAMG_FACE_CHAIN=0) and the
    per-step kernels (fused = 0) leave the default form's state, which is the oracle's"""
    a = gpu_solver(U8_53F, "P1", op=1)
    ref = oracle_state(U8_53F, "P1", a, op=1, solver=3)
    drive(a)
    sa = full_state(a)
    a.close()
    if form == "chain_off":
        monkeypatch.setenv("PAMG_FACE_CHAIN", "0")
    b = gpu_solver(U8_53F, "P1", op=1, fused=0 if form == "per_step" else 3)
    drive(b)
    sb = full_state(b)
    b.close()
    assert_states_equal(sb, sa, form)
    assert_states_equal(sb, ref, form)


# ---------------------------------------------------------------- sweep counts above 4
@gpu
@pytest.mark.parametrize("cycle", [0, 1])
@pytest.mark.parametrize("op", [0, 1])
@pytest.mark.parametrize("pset", ["default", "P1"])
@pytest.mark.parametrize("ns", [5, 7])
@pytest.mark.parametrize("shape", [U8_33, U8_53], ids=shape_id)
def test_sweep_counts_above_four_are_bitwise_the_oracle(shape, ns, pset, op, cycle):
    """n_smooth 5 and 7 (odd: k_face_pp's two-sweeps-per-pass leaves a single sweep over; the fused chains
    of n_smooth * n_coarse sweeps at counts the defaults never reach), fused 0 and 3"""
    for fused in (0, 3):
        g = gpu_solver(shape, pset, n_smooth=ns, op=op, cycle=cycle, fused=fused)
        ref = oracle_state(shape, pset, g, cycle=cycle, n_smooth=ns, op=op)
        drive(g)
        assert_states_equal(full_state(g), ref, f"fused={fused}")
        g.close()


# ---------------------------------------------------------------- roofline kernels, source term
@gpu
@pytest.mark.parametrize("pset", ["P1", "P2"])
@pytest.mark.parametrize("mesh,S", [("untitled8.msh", 3), ("irregular.msh", 3)])
def test_roofline_sweeps_match_oracle(mesh, S, pset):
    """k_sweep_stencil / k_sweep_assembled (tests/test_roofline_kernels.py) away from the defaults"""
    import pamg
    s = gpu_solver((mesh, S, 1), pset)
    o = O.Oracle(O.read_msh(path_of(mesh)), S, 1, **SETS[pset])
    rng = np.random.default_rng(20251019 + S)
    x, b = rng.uniform(-1, 1, (3, s.nsub(1), s.U)), rng.uniform(-1, 1, (3, s.nsub(1), s.U))
    s.set(pamg.TNEW_NONLIN, 1, x)
    s.set(pamg.RHS, 1, b)
    np.testing.assert_array_equal(s.sweep_bench_output(False), o.sweep_once(1, 0, x, b))
    np.testing.assert_array_equal(s.sweep_bench_output(True), o.sweep_once(1, 1, x, b))
    s.close()


@gpu
@pytest.mark.parametrize("pset", ["P1", "P2"])
def test_device_source_term_matches_the_host_sine(pset):
    """s' with the device sin vs the oracle's with the host libm sin: 1e-15 of its scale (k and dt scale it)"""
    import pamg
    g = gpu_solver(("test_sn2.msh", 3, 1), pset)
    o = O.Oracle(O.read_msh(path_of("test_sn2.msh")), 3, 1, ntime=1, n_multigrid=1, **SETS[pset])
    o.run()
    assert goldens.rel_err(g.get(pamg.SOURCE, 1), o.get(O.SOURCE, 1)) <= 1e-15
    g.close()


# ---------------------------------------------------------------- partitions
@gpu
@pytest.mark.parametrize("op", [0, 1])
def test_local_group_matches_single_domain_at_p1(op):
    """(untitled8, S 3, L 3) on two x-strips through the multi-rank exchange path (tests/test_multirank.py):
    op = 0 as the resident call, op = 1 with its agglomerated coarsest level, which runs n_coarse calls"""
    from pamg.solver import local_group, run_ranks
    import pamg
    mesh, S, L = U8_33
    m = pamg.Mesh.read(path_of(mesh))
    full = pamg.SemiImplicitIterative(m, S, L, op=op, **P1)
    drive(full)
    owner = m.x_strip_owner(2)
    parts = [pamg.SemiImplicitIterative(m, S, L, op=op, comm=(2, r, None, owner), **P1) for r in range(2)]
    local_group(parts)
    run_ranks(parts, drive)
    ref = full_state(full)
    for r, p in enumerate(parts):
        own = np.flatnonzero(owner == r)
        assert p.U == len(own)
        for k, v in full_state(p).items():
            np.testing.assert_array_equal(v, ref[k][:, :, own], err_msg=f"rank {r} {k}")
        p.close()
    full.close()
