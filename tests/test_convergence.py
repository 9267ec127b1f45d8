"""Convergence control: the device reductions (pamg_norm.hip) behind pamg_field_norm, pamg_get_convergence
(the reference's get_convergence, transport_tri_semi.F90:876-889), the read-only pamg_residual_norm and
pamg_solve, single domain and partitioned.

"Bitwise" is == on the float. The maxima are order-independent, so they are compared bitwise with numpy's.
The sum of squares is compared with math.fsum of the same (rounded) squares: a floating-point sum of n
non-negative terms in any order is within (n - 1) u of the exact sum, u = 2**-53, so L2**2 is held to
n * 2**-53 relative, n the number of entries -- derived, not measured.

No owner map of tests/test_multirank.py leaves a rank empty, so the empty-rank case of field_norm is not
repeated here (the library's own path for it, a level with N == 0, launches nothing and joins the identities).
"""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import goldens
import oracle_lib as O
from test_parameters import P1, P2, full_state

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U8_33, U8_53, IRR_33 = ("untitled8.msh", 3, 3), ("untitled8.msh", 5, 3), ("irregular.msh", 3, 3)


def path_of(mesh):
    return os.path.join(goldens.MESHES, mesh)


def solver(shape, **kw):
    import pamg
    mesh, S, L = shape
    return pamg.SemiImplicitIterative(pamg.Mesh.read(path_of(mesh)), S, L, **kw)


def expected(a):
    """(REF, MAXABS, sum of squares) of a host array, the last as the correctly rounded sum of the squares"""
    a = np.asarray(a, np.float64).ravel()
    return max(0.0, float(a.max())), float(np.abs(a).max()), math.fsum((a * a).tolist())


def assert_l2(l2, sumsq, n, what=""):
    assert abs(l2 * l2 - sumsq) <= n * 2.0 ** -53 * sumsq, (what, l2 * l2, sumsq, n)


def assert_norms(s, what, level, a, tag=""):
    import pamg
    ref, mx, ss = expected(a)
    assert s.field_norm(what, level, pamg.NORM_REF) == ref, (tag, "REF")
    assert s.field_norm(what, level, pamg.NORM_MAXABS) == mx, (tag, "MAXABS")
    assert_l2(s.field_norm(what, level, pamg.NORM_L2), ss, a.size, tag)


def assert_states_equal(got, ref, what=""):
    assert set(ref) == set(got)
    for k, v in ref.items():
        np.testing.assert_array_equal(got[k], v, err_msg=f"{what} {k}")


# ---------------------------------------------------------------- CPU: the header and the binding
def test_header_declares_the_norm_kinds_and_the_timing_class():
    from pamg import _lib
    text = open(os.path.join(ROOT, "include", "pamg.h")).read()
    for name, val in (("PAMG_NORM_REF", 0), ("PAMG_NORM_MAXABS", 1), ("PAMG_NORM_L2", 2)):
        m = re.search(r"#define\s+%s\s+(\d+)" % name, text)
        assert m and int(m.group(1)) == val, name
    assert (_lib.NORM_REF, _lib.NORM_MAXABS, _lib.NORM_L2) == (0, 1, 2)
    count = int(re.search(r"#define\s+PAMG_K_COUNT\s+(\d+)", text).group(1))
    assert len(_lib.K_NAMES) == count
    assert int(re.search(r"#define\s+PAMG_K_NORM\s+(\d+)", text).group(1)) == _lib.K_NAMES.index("norm")


# ---------------------------------------------------------------- 1. planted extrema
FIELD_SHAPES = [("one_tri.msh", 1, 1, (1,)), ("untitled8.msh", 3, 3, (1, 2, 3)), ("irregular.msh", 3, 3, (1, 2, 3)),
                ("900_ele.msh", 2, 2, (1,)), ("untitled8.msh", 5, 3, (1,))]


@gpu
@pytest.mark.parametrize("mesh,S,L,levels", FIELD_SHAPES, ids=[f"{m.split('.')[0]}-S{S}-L{L}" for m, S, L, _ in FIELD_SHAPES])
def test_field_norm_finds_planted_extrema(mesh, S, L, levels):
    """N = 4 (two threads), 512 / 128 / 32 (less than a wave), several workgroups with a partly filled last
    one; the extremum at the first and last entry, the last entry of each component, the first of the second
    un_ele -- and, on levels of at most 128 sub-elements, at every entry in turn (every storage position)"""
    import pamg
    s = solver((mesh, S, L))
    rng = np.random.default_rng(20261019)
    for l in levels:
        nsub, U = s.nsub(l), s.U
        base = rng.uniform(-1.0, 1.0, (3, nsub, U))
        s.set(pamg.RESIDUAL, l, base)
        assert_norms(s, pamg.RESIDUAL, l, base, f"L{l} base")
        spots = [(0, 0, 0), (2, nsub - 1, U - 1), (0, nsub - 1, U - 1), (1, nsub - 1, U - 1)]
        if U > 1:
            spots.append((0, 0, 1))
        for spot in spots:
            for v in (3.0, -5.0, 7.25):   # the largest value; the most negative; the largest magnitude
                a = base.copy()
                a[spot] = v
                if v == 7.25:
                    a[spot] = -v
                    a[(spot[0] + 1) % 3, spot[1], spot[2]] = 3.0
                s.set(pamg.RESIDUAL, l, a)
                assert_norms(s, pamg.RESIDUAL, l, a, f"L{l} {spot} {v}")
        if nsub * U <= 128:
            for i in range(base.size):
                a = base.copy().reshape(-1, order="F")
                a[i] = 2.0 + i
                a = a.reshape(base.shape, order="F")
                s.set(pamg.RESIDUAL, l, a)
                assert s.field_norm(pamg.RESIDUAL, l, pamg.NORM_REF) == 2.0 + i, i
                a[np.unravel_index(i, base.shape, order="F")] = -(2.0 + i)
                s.set(pamg.RESIDUAL, l, a)
                assert s.field_norm(pamg.RESIDUAL, l, pamg.NORM_MAXABS) == 2.0 + i, i
                assert s.field_norm(pamg.RESIDUAL, l, pamg.NORM_REF) == max(0.0, float(a.max())), i
        neg = -np.abs(base) - 0.125
        s.set(pamg.RESIDUAL, l, neg)
        assert s.field_norm(pamg.RESIDUAL, l, pamg.NORM_REF) == 0.0
        assert s.field_norm(pamg.RESIDUAL, l, pamg.NORM_MAXABS) == float(np.abs(neg).max())
        for spot in (spots[0], spots[1], (1, nsub // 2, U // 2)):
            for bad in (np.nan, np.inf, -np.inf):
                a = base.copy()
                a[spot] = bad
                s.set(pamg.RESIDUAL, l, a)
                for kind in (pamg.NORM_REF, pamg.NORM_MAXABS, pamg.NORM_L2):
                    assert math.isnan(s.field_norm(pamg.RESIDUAL, l, kind)), (l, spot, bad, kind)
        # the other selectors reduce their own field, and nothing was written by any of the calls
        s.set(pamg.RESIDUAL, l, base)
        other = rng.uniform(-2.0, 2.0, (3, nsub, U))
        for what in (pamg.TNEW, pamg.TOLD, pamg.RHS):
            s.set(what, l, other)
            assert_norms(s, what, l, other, f"L{l} field {what}")
            np.testing.assert_array_equal(s.get(what, l), other)
        np.testing.assert_array_equal(s.get(pamg.RESIDUAL, l), base)
    src = s.get(pamg.SOURCE, 1)
    assert_norms(s, pamg.SOURCE, 1, src, "source")
    tnn = s.get(pamg.TNEW_NONLIN)
    assert_norms(s, pamg.TNEW_NONLIN, 1, tnn, "tnew_nonlin")
    if L > 1:
        with pytest.raises(pamg.PamgError) as e:
            s.field_norm(pamg.SOURCE, 2, pamg.NORM_REF)
        assert e.value.rc == -1
    s.close()


# ---------------------------------------------------------------- 2. residual_norm: get_residual reduced, read-only
RESID_CASES = ([(U8_33, dict(arith=a, cycle=c, solver=sv)) for a in (0, 1) for c in (0, 1) for sv in (1, 3)] +
               [(U8_53, dict(P1)), (IRR_33, dict(P1))])


def _case_id(case):
    shape, kw = case
    return "{}-S{}-L{}-".format(shape[0].split(".")[0], shape[1], shape[2]) + \
        ("P1" if "dt" in kw else "a{arith}c{cycle}s{solver}".format(**kw))


@gpu
@pytest.mark.parametrize("case", RESID_CASES, ids=_case_id)
def test_residual_norm_is_get_residual_reduced_and_read_only(case):
    import pamg
    shape, kw = case
    a, b, c = (solver(shape, **kw) for _ in range(3))
    for x in (a, b, c):
        x.begin_timestep()
        x.vcycle(2)
    for l in range(1, shape[2] + 1):
        b.get_residual(l)
        r = b.get(pamg.RESIDUAL, l)
        ref, mx, ss = expected(r)
        assert a.residual_norm(l, pamg.NORM_REF) == ref, l
        assert a.residual_norm(l, pamg.NORM_MAXABS) == mx, l
        assert_l2(a.residual_norm(l, pamg.NORM_L2), ss, r.size, f"L{l}")
    assert_states_equal(full_state(a), full_state(c), "after residual_norm")
    a.vcycle(2)
    c.vcycle(2)
    assert_states_equal(full_state(a), full_state(c), "after residual_norm and two more cycles")
    for x in (a, b, c):
        x.close()


# ---------------------------------------------------------------- 3. get_convergence is the oracle's
@gpu
@pytest.mark.parametrize("shape", [U8_33, IRR_33], ids=["untitled8-S3-L3", "irregular-S3-L3"])
def test_get_convergence_is_the_oracles(shape):
    import pamg
    mesh, S, L = shape
    g, g2 = solver(shape), solver(shape)
    o = O.Oracle(O.read_msh(path_of(mesh)), S, L)
    o.set_source(g.get(pamg.SOURCE, 1))
    o.begin_timestep()
    for x in (g, g2):
        x.begin_timestep()
        x.vcycle(2)
    o.vcycle()
    o.vcycle()
    for l in range(1, L + 1):
        o.get_residual(l)
        g2.get_residual(l)
        assert g.get_convergence(l) == max(0.0, float(o.get(O.RES, l).max())), l
    sg = full_state(g)
    assert_states_equal(sg, full_state(g2), "get_convergence vs get_residual")
    assert_states_equal(sg, full_state(o), "vs oracle")
    g.close()
    g2.close()


@gpu
def test_ref_and_maxabs_differ_on_irregular_after_one_cycle():
    """irregular S3 L3 at the defaults after one cycle: max r = 2.177e-4, max |r| = 2.188e-4 on the oracle, so a
    swapped kind shows"""
    import pamg
    mesh, S, L = IRR_33
    g = solver(IRR_33)
    o = O.Oracle(O.read_msh(path_of(mesh)), S, L)
    o.set_source(g.get(pamg.SOURCE, 1))
    for x in (g, o):
        x.begin_timestep()
        x.vcycle()
    o.get_residual(1)
    r = o.get(O.RES, 1)
    ref, mx = max(0.0, float(r.max())), float(np.abs(r).max())
    assert ref != mx and abs(ref - 2.177e-4) < 1e-7 and abs(mx - 2.188e-4) < 1e-7, (ref, mx)
    assert g.get_convergence(1) == ref
    assert g.field_norm(pamg.RESIDUAL, 1, pamg.NORM_MAXABS) == mx
    assert g.field_norm(pamg.RESIDUAL, 1, pamg.NORM_REF) == ref
    g.close()


# ---------------------------------------------------------------- 4. solve
def _reference_run(shape, calls, kind, **kw):
    """a twin driven by vcycle(n) + residual_norm(1, kind) for n in calls: (values, states after each call)"""
    t = solver(shape, **kw)
    t.begin_timestep()
    vals, states = [], []
    for n in calls:
        t.vcycle(n)
        vals.append(t.residual_norm(1, kind))
        states.append(full_state(t))
    t.close()
    return vals, states


@gpu
@pytest.mark.parametrize("cycle", [0, 1])
def test_solve_stops_where_the_twin_says(cycle):
    import pamg
    ref, states = _reference_run(U8_33, [2, 2, 2, 2], pamg.NORM_MAXABS, cycle=cycle)
    print("MAXABS after 2/4/6/8 cycles:", ref)
    assert all(ref[i + 1] < ref[i] for i in range(3)), ref   # the condition the cases below rely on
    tol = math.sqrt(ref[1] * ref[2])
    s = solver(U8_33, cycle=cycle)
    s.begin_timestep()
    cycles, value, status, history = s.solve(tol, 8, check_every=2, kind=pamg.NORM_MAXABS)
    assert (cycles, status) == (6, pamg.SOLVE_CONVERGED)
    assert history == ref[:3] and value == ref[2]
    assert_states_equal(full_state(s), states[2], "solve vs three vcycle(2)")
    s.close()
    # a monitored run: tol < 0 never stops
    s = solver(U8_33, cycle=cycle)
    s.begin_timestep()
    cycles, value, status, history = s.solve(-1.0, 8, check_every=2)
    assert (cycles, status) == (8, pamg.SOLVE_MAXCYCLES) and history == ref and value == ref[3]
    assert_states_equal(full_state(s), states[3], "monitored run")
    s.close()
    # a short history array: two entries written, all four checks counted, the rest of the array untouched
    s = solver(U8_33, cycle=cycle)
    s.begin_timestep()
    hist = np.full(5, -7.0)
    cyc, st, nh, v = C.c_int(), C.c_int(), C.c_int(), C.c_double()
    s._call("pamg_solve", pamg.NORM_MAXABS, -1.0, 8, 2, C.byref(cyc), C.byref(v), C.byref(st), hist.ctypes.data, 2,
            C.byref(nh))
    assert (cyc.value, st.value, nh.value) == (8, pamg.SOLVE_MAXCYCLES, 4)
    assert list(hist) == ref[:2] + [-7.0] * 3 and v.value == ref[3]
    s.close()


@gpu
def test_solve_splits_the_cycles_into_calls_of_check_every():
    import pamg
    ref, states = _reference_run(U8_33, [3, 3, 2], pamg.NORM_MAXABS)
    s = solver(U8_33)
    s.begin_timestep()
    cycles, value, status, history = s.solve(-1.0, 8, check_every=3)
    assert (cycles, status) == (8, pamg.SOLVE_MAXCYCLES) and history == ref
    assert_states_equal(full_state(s), states[2], "calls of 3, 3, 2")
    # no cycles: no check, the state untouched
    r = s.solve(1.0, 0)
    assert r[0] == 0 and math.isnan(r[1]) and r[2] == pamg.SOLVE_MAXCYCLES and r[3] == []
    assert_states_equal(full_state(s), states[2], "max_cycles = 0")
    s.close()


@gpu
def test_solve_reports_a_run_that_does_not_converge():
    """irregular S3 L3 at P2 (the diffusion term dominates): max |r| never falls below 6e-3 in 8 cycles (on the
    oracle it grows to 7e-2)"""
    import pamg
    s = solver(IRR_33, **P2)
    s.begin_timestep()
    cycles, value, status, history = s.solve(1e-3, 8, check_every=2)
    print("P2 history:", history)
    assert (cycles, status) == (8, pamg.SOLVE_MAXCYCLES) and len(history) == 4
    assert min(history) >= 6e-3
    s.close()


@gpu
def test_solve_stops_at_a_non_finite_value():
    import pamg
    s = solver(U8_33)
    s.begin_timestep()
    t = s.get(pamg.TNEW, 1)
    t[1, 5, 3] = np.nan
    s.set(pamg.TNEW, 1, t)
    cycles, value, status, history = s.solve(1e-3, 8, check_every=2)
    assert (cycles, status) == (2, pamg.SOLVE_NONFINITE)
    assert math.isnan(value) and len(history) == 1 and math.isnan(history[0])
    s.close()


# ---------------------------------------------------------------- 5. refusals
@gpu
@pytest.mark.parametrize("kw", [dict(op=1), dict(solver=2)], ids=["op1", "solver2"])
def test_read_only_form_is_refused_where_the_residual_writes(kw):
    import pamg
    s, t = solver(U8_33, **kw), solver(U8_33, **kw)
    for x in (s, t):
        x.begin_timestep()
        x.vcycle(1)
    for call in (lambda: s.residual_norm(1, pamg.NORM_MAXABS), lambda: s.solve(1e-3, 4)):
        with pytest.raises(pamg.PamgError) as e:
            call()
        assert e.value.rc == -1 and "read-only" in str(e.value)
    assert_states_equal(full_state(s), full_state(t), "a refused call changed the state")
    # the stored-field forms work for every configuration
    for l in (1, 3):
        t.get_residual(l)
        r = t.get(pamg.RESIDUAL, l)
        assert s.get_convergence(l) == max(0.0, float(r.max()))
        assert_norms(s, pamg.RESIDUAL, l, r, f"L{l}")
    assert_states_equal(full_state(s), full_state(t), "get_convergence vs get_residual")
    s.close()
    t.close()


@gpu
def test_bad_arguments_are_refused():
    import pamg
    s = solver(U8_33)
    s.begin_timestep()
    before = full_state(s)
    bad = [lambda: s.residual_norm(1, 3), lambda: s.residual_norm(1, -1), lambda: s.field_norm(pamg.RESIDUAL, 1, 7),
           lambda: s.field_norm(9, 1, pamg.NORM_REF), lambda: s.residual_norm(4, pamg.NORM_REF),
           lambda: s.solve(1e-3, 8, check_every=0), lambda: s.solve(1e-3, -1), lambda: s.solve(1e-3, 8, kind=5)]
    for call in bad:
        with pytest.raises(pamg.PamgError) as e:
            call()
        assert e.value.rc == -1
    assert_states_equal(full_state(s), before, "a refused call changed the state")
    s.close()


# ---------------------------------------------------------------- 6. partitions
@gpu
@pytest.mark.parametrize("nparts", [2, 4])
def test_partitioned_norms_and_solve_are_the_single_domains(nparts):
    import pamg
    from pamg.solver import local_group, run_ranks
    mesh, S, L = U8_33
    m = pamg.Mesh.read(path_of(mesh))
    kinds = (pamg.NORM_REF, pamg.NORM_MAXABS, pamg.NORM_L2)

    def drive(x, out):
        x.begin_timestep()
        x.vcycle(2)
        out["norm"] = {(l, k): x.residual_norm(l, k) for l in range(1, L + 1) for k in kinds}
        out["solve"] = x.solve(out["tol"], 8, check_every=2) if "tol" in out else None
        out["conv"] = [x.get_convergence(l) for l in range(1, L + 1)]
        out["field"] = [x.field_norm(pamg.TNEW, l, pamg.NORM_MAXABS) for l in range(1, L + 1)]

    full = pamg.SemiImplicitIterative(m, S, L)
    probe = pamg.SemiImplicitIterative(m, S, L)   # the tolerance: between the 2nd and 3rd check after the first two cycles
    probe.begin_timestep()
    probe.vcycle(2)
    h = probe.solve(-1.0, 8, check_every=2)[3]
    assert h[0] > h[1] > h[2]
    probe.close()
    ref = dict(tol=math.sqrt(h[1] * h[2]), ss={})
    drive(full, ref)
    assert ref["solve"][0] == 6 and ref["solve"][2] == pamg.SOLVE_CONVERGED
    for l in range(1, L + 1):   # the single domain's own values are get_residual's
        chk = pamg.SemiImplicitIterative(m, S, L)
        chk.begin_timestep()
        chk.vcycle(2)
        chk.get_residual(l)
        e = expected(chk.get(pamg.RESIDUAL, l))
        assert (ref["norm"][l, pamg.NORM_REF], ref["norm"][l, pamg.NORM_MAXABS]) == e[:2]
        ref["ss"][l] = e[2]
        chk.close()

    owner = m.x_strip_owner(nparts)
    parts = [pamg.SemiImplicitIterative(m, S, L, comm=(nparts, r, None, owner)) for r in range(nparts)]
    local_group(parts)
    outs = {id(p): dict(tol=ref["tol"]) for p in parts}
    run_ranks(parts, lambda p: drive(p, outs[id(p)]))
    n_entries = 3 * m.U
    for l in range(1, L + 1):
        assert_l2(ref["norm"][l, pamg.NORM_L2], ref["ss"][l], n_entries * full.nsub(l), f"single domain L{l}")
    for r, p in enumerate(parts):
        out = outs[id(p)]
        for (l, k), v in out["norm"].items():
            if k == pamg.NORM_L2:
                assert_l2(v, ref["ss"][l], n_entries * p.nsub(l), f"rank {r} L{l}")
                assert v == outs[id(parts[0])]["norm"][l, k], "every rank receives the same double"
            else:
                assert v == ref["norm"][l, k], (r, l, k)
        assert out["solve"][0] == ref["solve"][0] and out["solve"][2:] == ref["solve"][2:], (r, out["solve"])
        assert out["solve"][1] == ref["solve"][1]
        assert out["conv"] == ref["conv"] and out["field"] == ref["field"], r
    ref_state, ref_ov = full.state(), full.overlap()
    for r, p in enumerate(parts):
        own = np.flatnonzero(owner == r)
        for k, v in p.state().items():
            np.testing.assert_array_equal(v, ref_state[k][:, :, own], err_msg=f"rank {r} {k}")
        for x, y in zip(p.overlap(), ref_ov):
            np.testing.assert_array_equal(x, y[:, :, own], err_msg=f"rank {r} t_overlap")
        p.close()
    full.close()


@gpu
def test_detached_partition_returns_its_local_value():
    import pamg
    mesh, S, L = U8_33
    m = pamg.Mesh.read(path_of(mesh))
    owner = m.x_strip_owner(2)
    p = pamg.SemiImplicitIterative(m, S, L, comm=(2, 1, None, owner))
    a = np.random.default_rng(5).uniform(-1, 1, (3, p.nsub(1), p.U))
    p.set(pamg.RESIDUAL, 1, a)
    assert_norms(p, pamg.RESIDUAL, 1, a, "detached")
    p.close()


@gpu
def test_self_peer_norms_cross_the_rccl_gather():
    """a one-rank RCCL communicator (tests/test_rccl_self.py): the record goes through ncclAllGather"""
    import pamg
    mesh, S, L = U8_33
    m = pamg.Mesh.read(path_of(mesh))
    full = pamg.SemiImplicitIterative(m, S, L)
    s = pamg.SemiImplicitIterative(m, S, L, self_peer=(pamg.unique_id(), m.x_strip_owner(2)))
    assert s.comm_info()[0] == "rccl"
    res = []
    for x in (full, s):
        x.begin_timestep()
        x.vcycle(2)
        v = [x.residual_norm(l, k) for l in range(1, L + 1) for k in (pamg.NORM_REF, pamg.NORM_MAXABS, pamg.NORM_L2)]
        v.append(x.solve(-1.0, 4, check_every=2))
        v += [x.get_convergence(l) for l in range(1, L + 1)]
        res.append(v)
    assert res[0] == res[1]
    assert_states_equal(full_state(s), full_state(full), "self-peer")
    s.close()
    full.close()


# ---------------------------------------------------------------- 7. the Fortran host
@gpu
def test_fortran_host_solves_to_a_tolerance(tmp_path):
    import pamg
    import pamg_records
    ref, states = _reference_run(U8_33, [2, 2, 2, 2], pamg.NORM_MAXABS)
    assert ref[1] > ref[2]
    tol = math.sqrt(ref[1] * ref[2])
    shutil.copy(path_of("untitled8.msh"), tmp_path)
    (tmp_path / "pamg_run.nml").write_text(
        "&transport mesh_file='untitled8.msh', n_split=3, multi_levels=3, n_smooth=4, solver=3, ntime=1,\n"
        f" n_multigrid=8, device=0, dump='out.bin', call_sites=0, solve_tol={tol!r}, check_every=2 /\n")
    exe = os.path.join(ROOT, "p-a_multigrids_amd", "bin", "pamg_transport")
    r = subprocess.run([exe], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"convergence\s+(\S+)\s+cycles\s+(\d+)\s+status\s+(\d+)", r.stdout)
    assert m, r.stdout
    assert int(m.group(2)) == 6 and int(m.group(3)) == pamg.SOLVE_CONVERGED
    assert abs(float(m.group(1)) - ref[2]) <= 1e-12 * ref[2]
    got = pamg_records.read_records(str(tmp_path / "out.bin"))
    assert_states_equal(got, states[2], "host dump vs python twin")
