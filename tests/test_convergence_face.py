"""Convergence control of the face operator (op = 1): pamg_params.monitor = 1 gives the handle a monitor halo
image of its own, so that pamg_residual_norm and pamg_solve reduce the face-coupled residual A tnew - RHS
(k_face_residual_reduce, pamg_face.hip) without storing it or touching t_overlap, single domain and partitioned.

The yardstick is the stored path on a twin without the monitor: pamg_get_residual(level), read back, reduced
by numpy. "Bitwise" is == on the float. The maxima are order-independent and compared bitwise; the sum of
squares is held to n * 2**-53 relative of math.fsum of the same squares, the bound tests/test_convergence.py
derives (n entries, any summation order).

Shapes: (untitled8, 3, 3) has 64 / 16 / 4 sub-elements per un_ele, so level 1 runs the wave-uniform instance
of the reduction and levels 2 and 3 the other; (untitled8, 2, 2) has a level 1 that is not wave-uniform;
(untitled8_rn, 3, 3) and (irregular, 3, 3) reach the 18 (face, fNeig, Dir) triples, reversed faces included
(tests/test_face_model.py), which is where the monitor's slot arithmetic could differ from halo_face's.

No owner map used here leaves a rank without un_eles (x_strip_owner splits untitled8's 8 un_eles 4 + 4 or
2 + 2 + 2 + 2), so the empty-rank case is not constructed: the library's path for it launches nothing, joins
the identities and still takes part in the gather.
"""
import inspect
import math
import os
import re

import numpy as np
import pytest

from test_convergence import assert_l2, assert_states_equal, expected, path_of, solver
from test_parameters import P1, full_state

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U8_33, U8RN_33, IRR_33, U8_22 = (("untitled8.msh", 3, 3), ("untitled8_rn.msh", 3, 3), ("irregular.msh", 3, 3),
                                 ("untitled8.msh", 2, 2))


# ---------------------------------------------------------------- 1. CPU: the field and its mirrors
def test_monitor_takes_the_place_of_reserved_in_every_mirror():
    import ctypes as C

    import pamg
    from pamg import _lib
    text = open(os.path.join(ROOT, "include", "pamg.h")).read()
    body = re.search(r"typedef struct \{(.*?)\}\s*pamg_params;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    assert decls[-2:] == ["int op", "int monitor"], decls[-3:]
    assert "reserved" not in body
    names = [n for n, _ in _lib.PamgParams._fields_]
    assert names[-2:] == ["op", "monitor"] and "reserved" not in names
    assert dict(_lib.PamgParams._fields_)["monitor"] is C.c_int
    assert [d.split()[-1].split("[")[0] for d in decls] == names          # the same fields in the same order
    assert C.sizeof(_lib.PamgParams) == 6 * 4 + 4 * 8 + 8 * 4              # the size did not change
    assert _lib.PamgParams.monitor.offset == C.sizeof(_lib.PamgParams) - 4
    f90 = open(os.path.join(ROOT, "p-a_multigrids_amd", "fortran", "pamg_mod.F90")).read()
    ftype = re.search(r"type, bind\(C\), public :: pamg_params(.*?)end type pamg_params", f90, flags=re.S).group(1)
    comps = [c.strip() for ln in ftype.strip().splitlines() for c in ln.split("::")[1].split(",")]
    assert comps == names, comps
    assert re.search(r"integer\(c_int\) :: monitor\s*$", ftype.rstrip())
    assert pamg.default_params().monitor == 0
    assert pamg.default_params(monitor=1).monitor == 1
    assert inspect.signature(pamg.SemiImplicitIterative.__init__).parameters["monitor"].default == 0


# ---------------------------------------------------------------- 2. value and read-only, single domain
VALUE_CASES = ([(shape, dict(solver=sv, cycle=c)) for shape in (U8_33, U8RN_33, IRR_33, U8_22) for sv in (1, 3)
                for c in (0, 1)] +
               [(U8_33, dict(P1, solver=3, cycle=0)), (U8RN_33, dict(P1, solver=1, cycle=1)),
                (IRR_33, dict(P1, solver=3, cycle=1)), (U8_22, dict(P1, solver=1, cycle=0))])


def _case_id(case):
    shape, kw = case
    return "{}-S{}-L{}-{}s{}c{}".format(shape[0].split(".")[0], shape[1], shape[2], "P1" if "dt" in kw else "",
                                        kw["solver"], kw["cycle"])


def _check_levels(a, b, levels, tag=""):
    """a's read-only norms of every level against numpy's reduction of the residual b stores"""
    import pamg
    for l in levels:
        b.get_residual(l)
        r = b.get(pamg.RESIDUAL, l)
        ref, mx, ss = expected(r)
        ga, gm, gl = (a.residual_norm(l, k) for k in (pamg.NORM_REF, pamg.NORM_MAXABS, pamg.NORM_L2))
        print(f"{tag} L{l}: REF {ga!r} / {ref!r}  MAXABS {gm!r} / {mx!r}  L2^2 {gl * gl!r} / {ss!r}")
        assert ga == ref, (tag, l, "REF")
        assert gm == mx, (tag, l, "MAXABS")
        assert_l2(gl, ss, r.size, f"{tag} L{l}")


@gpu
@pytest.mark.parametrize("case", VALUE_CASES, ids=_case_id)
def test_face_residual_norm_is_get_residual_reduced_and_read_only(case):
    shape, kw = case
    a = solver(shape, op=1, monitor=1, **kw)
    b, c = (solver(shape, op=1, **kw) for _ in range(2))
    for x in (a, b, c):
        x.begin_timestep()
        x.vcycle(2)
    _check_levels(a, b, range(1, shape[2] + 1), _case_id(case))
    assert_states_equal(full_state(a), full_state(c), "after residual_norm")
    a.vcycle(2)
    c.vcycle(2)
    assert_states_equal(full_state(a), full_state(c), "after residual_norm and two more cycles")
    for x in (a, b, c):
        x.close()


@gpu
def test_words_of_another_level_do_not_leak_into_a_check():
    """the monitor image is shared by the levels: level 1's value after level-2 and level-3 checks filled the
    image is the value of a handle whose image never held another level's words, and level 2's value is the
    same before and after a level-1 check"""
    import pamg
    a, d = (solver(U8_33, op=1, monitor=1, solver=3) for _ in range(2))
    for x in (a, d):
        x.begin_timestep()
        x.vcycle(2)
    first2 = [d.residual_norm(2, k) for k in (pamg.NORM_REF, pamg.NORM_MAXABS, pamg.NORM_L2)]
    d.residual_norm(3, pamg.NORM_MAXABS)
    for k in (pamg.NORM_REF, pamg.NORM_MAXABS, pamg.NORM_L2):
        assert d.residual_norm(1, k) == a.residual_norm(1, k), k
    assert [d.residual_norm(2, k) for k in (pamg.NORM_REF, pamg.NORM_MAXABS, pamg.NORM_L2)] == first2
    a.close()
    d.close()


# ---------------------------------------------------------------- 3. the face terms are in the value
@gpu
def test_face_coupling_is_in_the_value():
    """the same tnew and RHS under the block-diagonal operator give another residual: a monitor that dropped the
    face terms would return op = 0's value"""
    import pamg
    f = solver(IRR_33, op=1, monitor=1)
    f.begin_timestep()
    f.vcycle(1)
    g = solver(IRR_33)
    g.set(pamg.TNEW, 1, f.get(pamg.TNEW, 1))
    g.set(pamg.RHS, 1, f.get(pamg.RHS, 1))
    vf, vg = f.residual_norm(1, pamg.NORM_MAXABS), g.residual_norm(1, pamg.NORM_MAXABS)
    print("op = 1:", vf, " op = 0 on the same tnew, RHS:", vg)
    assert vf != vg
    f.close()
    g.close()


# ---------------------------------------------------------------- 4. solve
def _twin_values(shape, ncalls, **kw):
    """no-monitor twins, one per number of vcycle(2) calls: max |r| of get_residual(1) after 1 .. ncalls calls,
    and the states right before the residual was stored"""
    import pamg
    vals, states = [], []
    for n in range(1, ncalls + 1):
        t = solver(shape, op=1, **kw)
        t.begin_timestep()
        for _ in range(n):
            t.vcycle(2)
        states.append(full_state(t))
        t.get_residual(1)
        vals.append(float(np.abs(t.get(pamg.RESIDUAL, 1)).max()))
        t.close()
    return vals, states


@gpu
@pytest.mark.parametrize("cycle", [0, 1])
def test_face_solve_stops_where_the_twins_say(cycle):
    import pamg
    ref, states = _twin_values(U8_33, 4, cycle=cycle)
    print("max |r| after 2/4/6/8 cycles:", ref)
    assert all(ref[i + 1] < ref[i] for i in range(3)), ref
    tol = math.sqrt(ref[1] * ref[2])
    s = solver(U8_33, op=1, monitor=1, cycle=cycle)
    s.begin_timestep()
    cycles, value, status, history = s.solve(tol, 8, check_every=2, kind=pamg.NORM_MAXABS)
    assert (cycles, value, status, history) == (6, ref[2], pamg.SOLVE_CONVERGED, ref[:3])
    assert_states_equal(full_state(s), states[2], "solve vs three vcycle(2)")
    s.close()
    s = solver(U8_33, op=1, monitor=1, cycle=cycle)
    s.begin_timestep()
    cycles, value, status, history = s.solve(-1.0, 8, check_every=2, kind=pamg.NORM_MAXABS)
    assert (cycles, status) == (8, pamg.SOLVE_MAXCYCLES) and len(history) == 4
    assert history == ref and value == ref[3]
    assert_states_equal(full_state(s), states[3], "monitored run")
    s.close()


@gpu
def test_face_solve_reports_a_run_that_does_not_converge():
    """irregular S3 L3, Jacobi, dt = 0.05, k = 3, the reference cycle: the oracle's max |r| after cycles 1..8 is
    0.49, 0.37, 0.38, 0.46, 0.60, 0.81, 1.13, 1.59"""
    import pamg
    s = solver(IRR_33, op=1, monitor=1, solver=1, dt=0.05, k=3.0, cycle=0)
    s.begin_timestep()
    cycles, value, status, history = s.solve(1e-3, 8, check_every=1)
    print("history:", history)
    assert (cycles, status) == (8, pamg.SOLVE_MAXCYCLES) and len(history) == 8 and value == history[-1]
    assert min(history) >= 0.3
    s.close()


@gpu
def test_face_solve_stops_at_a_non_finite_value():
    import pamg
    s = solver(U8_33, op=1, monitor=1)
    s.begin_timestep()
    t = s.get(pamg.TNEW, 1)
    t[1, 5, 3] = np.nan
    s.set(pamg.TNEW, 1, t)
    cycles, value, status, history = s.solve(1e-3, 8, check_every=2)
    assert (cycles, status) == (2, pamg.SOLVE_NONFINITE)
    assert math.isnan(value) and len(history) == 1 and math.isnan(history[0])
    s.close()


# ---------------------------------------------------------------- 5. refusals
def test_monitor_values_other_than_0_and_1_are_refused_before_the_device_is_looked_for():
    """pamg_create checks its parameters before it asks for a device: PAMG_ERR_ARG with or without a GPU"""
    import ctypes as C

    import pamg
    from pamg import _lib
    for v in (2, -1):
        h = C.c_void_p()
        p = pamg.default_params(n_split=3, multi_levels=3, op=1, monitor=v)
        assert _lib.lib().pamg_create(C.byref(p), C.byref(h)) == -1, v
        assert not h.value


def _refused(call, rc, word):
    import pamg
    with pytest.raises(pamg.PamgError) as e:
        call()
    assert e.value.rc == rc and word in str(e.value), str(e.value)


@gpu
def test_face_refusals_leave_the_state_untouched():
    import pamg
    from pamg.solver import local_group, run_ranks
    with pytest.raises(pamg.PamgError) as e:
        solver(U8_33, op=1, monitor=2)
    assert e.value.rc == -1
    # monitor = 0, op = 1: what tests/test_convergence.py pins; monitor = 1, op = 0, solver 2 stays refused
    for kw in (dict(op=1), dict(op=0, monitor=1, solver=2)):
        s, t = solver(U8_33, **kw), solver(U8_33, **kw)
        for x in (s, t):
            x.begin_timestep()
            x.vcycle(1)
        _refused(lambda: s.residual_norm(1, pamg.NORM_MAXABS), -1, "read-only")
        _refused(lambda: s.solve(1e-3, 4), -1, "read-only")
        assert_states_equal(full_state(s), full_state(t), f"a refused call changed the state {kw}")
        s.close()
        t.close()
    # monitor = 1 with op = 0 has no effect: the value is the plain handle's
    s, t = solver(U8_33, monitor=1), solver(U8_33)
    for x in (s, t):
        x.begin_timestep()
        x.vcycle(1)
    assert s.residual_norm(1, pamg.NORM_L2) == t.residual_norm(1, pamg.NORM_L2)
    assert_states_equal(full_state(s), full_state(t), "monitor = 1, op = 0")
    s.close()
    t.close()
    mesh, S, L = U8_33
    m = pamg.Mesh.read(path_of(mesh))
    owner = m.x_strip_owner(2)
    # a detached partition cannot see its peers' tnew
    p = pamg.SemiImplicitIterative(m, S, L, op=1, monitor=1, comm=(2, 1, None, owner))
    before = full_state(p)
    _refused(lambda: p.residual_norm(1, pamg.NORM_MAXABS), -4, "detached")
    _refused(lambda: p.solve(1e-3, 4), -4, "detached")
    assert_states_equal(full_state(p), before, "detached")
    p.close()
    # the agglomerated coarsest level of a bound partition
    parts = [pamg.SemiImplicitIterative(m, S, L, op=1, monitor=1, comm=(2, r, None, owner)) for r in range(2)]
    local_group(parts)

    def start(x):
        x.begin_timestep()
        x.vcycle(1)
    run_ranks(parts, start)
    before = [full_state(x) for x in parts]
    run_ranks(parts, lambda x: _refused(lambda: x.residual_norm(L, pamg.NORM_MAXABS), -1, "agglomerated"))
    for x, st in zip(parts, before):
        assert_states_equal(full_state(x), st, "agglomerated level")
        x.close()


# ---------------------------------------------------------------- 6. partitions (local group)
KINDS = (0, 1, 2)   # NORM_REF, NORM_MAXABS, NORM_L2


def _drive(x, out, levels):
    x.begin_timestep()
    x.vcycle(2)
    out["norm"] = {(l, k): x.residual_norm(l, k) for l in levels for k in KINDS}
    out["solve"] = x.solve(out["tol"], 8, check_every=2)


@gpu
@pytest.mark.parametrize("nparts", [2, 4])
def test_partitioned_face_norms_and_solve_are_the_single_domains(nparts):
    import pamg
    from pamg.solver import local_group, run_ranks
    mesh, S, L = U8_33
    m = pamg.Mesh.read(path_of(mesh))
    levels = (1, 2)   # level 3 is agglomerated on the partitions
    probe = pamg.SemiImplicitIterative(m, S, L, op=1, monitor=1)
    probe.begin_timestep()
    probe.vcycle(2)
    h = probe.solve(-1.0, 8, check_every=2)[3]
    assert h[0] > h[1] > h[2], h
    probe.close()
    full = pamg.SemiImplicitIterative(m, S, L, op=1, monitor=1)
    ref = dict(tol=math.sqrt(h[1] * h[2]))
    _drive(full, ref, levels)
    assert ref["solve"][0] == 6 and ref["solve"][2] == pamg.SOLVE_CONVERGED, ref["solve"]
    ss = {}
    for l in levels:   # the single domain's own values are get_residual's
        chk = pamg.SemiImplicitIterative(m, S, L, op=1)
        chk.begin_timestep()
        chk.vcycle(2)
        chk.get_residual(l)
        e = expected(chk.get(pamg.RESIDUAL, l))
        assert (ref["norm"][l, pamg.NORM_REF], ref["norm"][l, pamg.NORM_MAXABS]) == e[:2], l
        ss[l] = e[2]
        chk.close()

    owner = m.x_strip_owner(nparts)
    assert all((owner == r).any() for r in range(nparts))   # no rank is empty (the module's docstring)
    parts = [pamg.SemiImplicitIterative(m, S, L, op=1, monitor=1, comm=(nparts, r, None, owner))
             for r in range(nparts)]
    local_group(parts)
    outs = {id(p): dict(tol=ref["tol"]) for p in parts}
    run_ranks(parts, lambda p: _drive(p, outs[id(p)], levels))
    n_entries = 3 * m.U
    for r, p in enumerate(parts):
        out = outs[id(p)]
        for (l, k), v in out["norm"].items():
            if k == pamg.NORM_L2:
                assert_l2(v, ss[l], n_entries * p.nsub(l), f"rank {r} L{l}")
                assert v == outs[id(parts[0])]["norm"][l, k], "every rank receives the same double"
            else:
                assert v == ref["norm"][l, k], (r, l, k)
        # the maxima are the single domain's bit for bit, so the run stops at the same check with the same values
        assert out["solve"] == ref["solve"], (r, out["solve"], ref["solve"])

    def compare(tag):
        ref_state, ref_ov = full.state(), full.overlap()
        for r, p in enumerate(parts):
            own = np.flatnonzero(owner == r)
            for k, v in p.state().items():
                np.testing.assert_array_equal(v, ref_state[k][:, :, own], err_msg=f"{tag} rank {r} {k}")
            for x, y in zip(p.overlap(), ref_ov):
                np.testing.assert_array_equal(x, y[:, :, own], err_msg=f"{tag} rank {r} t_overlap")

    compare("after solve")
    full.vcycle(2)
    run_ranks(parts, lambda p: p.vcycle(2))
    compare("after two further cycles")
    for p in parts:
        p.close()
    full.close()


# ---------------------------------------------------------------- 7. the RCCL transport on one GPU
@gpu
def test_self_peer_face_monitor_crosses_rccl():
    """a one-rank RCCL communicator (tests/test_rccl_self.py): the monitor words across the two virtual parts go
    through ncclSend / ncclRecv, 3 per entry, and the record through ncclAllGather"""
    import pamg
    mesh, S, L = U8_33
    m = pamg.Mesh.read(path_of(mesh))
    full = pamg.SemiImplicitIterative(m, S, L, op=1, monitor=1)
    s = pamg.SemiImplicitIterative(m, S, L, op=1, monitor=1, self_peer=(pamg.unique_id(), m.x_strip_owner(2)))
    assert s.comm_info()[0] == "rccl"
    res = []
    for x in (full, s):
        x.begin_timestep()
        x.vcycle(2)
        v = [x.residual_norm(l, k) for l in (1, 2) for k in KINDS]
        v.append(x.solve(-1.0, 4, check_every=2))
        res.append(v)
    assert res[0] == res[1]
    assert_states_equal(full_state(s), full_state(full), "self-peer")
    s.close()
    full.close()
