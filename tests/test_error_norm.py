"""get_error on the device (transport_tri_semi.F90:531-540, called at :303): the error field
tracer(1)%error = |tnew - sin(x + y)| (pamg_get_error, selector ERROR), the same values reduced without being
stored (pamg_error_norm), and the two norms that came with them, NORM_L1 and NORM_L2_MASS, on every field.

Node coordinates for the numpy side are the library's own get_splitting in fp64: pamg_write_vtu's points read
back with tests/vtu_io.py. "Bitwise" is == on the float.

Bounds, derived and not measured (u = 2**-53):
 - error field against numpy: (3 R + 4) u with R = max(|x| + |y|) over the points -- at most 3 roundings in each
   coordinate sum (where the device's differ from the host's), sine is 1-Lipschitz, the device sine within 1 ulp
   of values at most 1, one rounding in the subtraction with |tnew| <= 1. The build does not contract (the
   library is compiled with -ffp-contract=off) and error_one repeats the host's get_splitting operation for
   operation, so the coordinates are in fact the host's bits and only the two sines differ: the measured maximum
   (printed by the test) is 2.2e-16 on every shape, against bounds of 8.0e-16 to 2.0e-14.
 - L1: a floating-point sum of n non-negative terms in any order is within (n - 1) u of the exact sum (the
   existing L2 argument of tests/test_convergence.py): n u relative against math.fsum.
 - L2_MASS: (n_sub + 32) u relative on the square, n_sub the sub-elements of the level: n_sub - 1 for the
   summation order, the rest for the few roundings in M_12 (detwei, w = 1/3) and in each term. The reference is
   exact (integers and fractions from the float inputs), with M_s = A_un / 4**i_split / 12 [[2,1,1],[1,2,1],[1,1,2]].
   M_12 of the oracle's stencil differs from A / 12 / 4**i_split by at most 1.98 ulp on these shapes (measured on
   the CPU by test_oracle_m12_is_the_area_over_12, which holds it to 8 ulp), so nothing is added to the bound.
"""
import json
import math
import os
import re
import shutil
import subprocess
import tempfile
from fractions import Fraction

import numpy as np
import pytest

import goldens
import oracle_lib as O
import vtu_io
from test_convergence import FIELD_SHAPES, assert_l2, assert_states_equal, expected, path_of, solver
from test_parameters import full_state

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "p-a_multigrids_amd", "bin", "pamg_transport")
U = 2.0 ** -53

SHAPES = list(FIELD_SHAPES) + [("untitled8_rn.msh", 3, 3, (1, 2, 3))]
IDS = [f"{m.split('.')[0]}-S{S}-L{L}" for m, S, L, _ in SHAPES]
KINDS = (0, 1, 2, 3, 4)
U8_33 = ("untitled8.msh", 3, 3)


# ---------------------------------------------------------------- helpers
_COORDS = {}


def coords(s, key):
    """x, y of the handle's level-1 nodes as (3, nsub, U): the points pamg_write_vtu writes (get_splitting, fp64)"""
    if key not in _COORDS:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "c.vtu")
            s.write_vtu(path)
            pts = vtu_io.read_vtu(path)["points"]
        shp = (3, s.nsub(1), s.U)
        _COORDS[key] = (pts[:, 0].reshape(shp, order="F").copy(), pts[:, 1].reshape(shp, order="F").copy())
    return _COORDS[key]


def field_bound(x, y):
    return (3.0 * float((np.abs(x) + np.abs(y)).max()) + 4.0) * U


def areas(X):
    """exact areas of the un_eles (the shoelace sum over mesh.X, (2, 3, U) column-major) as fractions"""
    out = []
    for c in np.asarray(X, np.float64).reshape(-1, 6):
        x0, y0, x1, y1, x2, y2 = (Fraction(float(v)) for v in c)
        out.append(abs((x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)) / 2)
    return out


def exact_ints(a):
    """(ints, k) with a == ints * 2**k exactly, ints an object array of Python integers"""
    a = np.asarray(a, np.float64)
    m, e = np.frexp(a.ravel())
    mi = (m * 2.0 ** 53).astype(np.int64)   # exact: |m| < 1 has 53 significant bits
    e = e.astype(np.int64) - 53
    k = int(e[mi != 0].min()) if (mi != 0).any() else 0
    ints = [(q << (s - k)) if q else 0 for q, s in zip(mi.tolist(), e.tolist())]
    return np.array(ints, dtype=object).reshape(a.shape), k


def mass_sq_exact(a, area, i_split):
    """sum_s v_s^T M_s v_s of a (3, nsub, U) field, exactly, with M_s = A_un / 4**i_split / 12 [[2,1,1],[1,2,1],[1,1,2]]"""
    v, k = exact_ints(a)
    q = (v[0] + v[1] + v[2]) ** 2 + v[0] ** 2 + v[1] ** 2 + v[2] ** 2   # (nsub, U)
    per_u = q.sum(axis=0)
    tot = sum((area[u] * int(per_u[u]) for u in range(len(area))), Fraction(0))
    return tot * Fraction(2) ** (2 * k) / 12 / 4 ** i_split


def assert_mass(value, exact, n_sub, what=""):
    """value**2 within (n_sub + 32) u of the exact square"""
    got = Fraction(value) ** 2
    assert abs(got - exact) <= Fraction(n_sub + 32) * Fraction(U) * exact, \
        (what, float(got), float(exact), float(abs(got - exact) / exact) / U if exact else 0.0, n_sub)


def assert_l1(value, a, what=""):
    ref = math.fsum(np.abs(np.asarray(a, np.float64)).ravel().tolist())
    assert abs(value - ref) <= a.size * U * ref, (what, value, ref)


def planted_spots(nsub, Uloc):
    spots = [(0, 0, 0), (2, nsub - 1, Uloc - 1), (0, nsub - 1, Uloc - 1), (1, nsub - 1, Uloc - 1)]
    if Uloc > 1:
        spots.append((0, 0, 1))
    return spots


# ---------------------------------------------------------------- 1. CPU: header and binding
def test_header_declares_the_error_selector_and_the_new_kinds():
    import pamg
    from pamg import _lib
    text = open(os.path.join(ROOT, "include", "pamg.h")).read()
    for name, val in (("PAMG_ERROR", 6), ("PAMG_NORM_L1", 3), ("PAMG_NORM_L2_MASS", 4)):
        m = re.search(r"#define\s+%s\s+(\d+)" % name, text)
        assert m and int(m.group(1)) == val, name
    assert (_lib.ERROR, _lib.NORM_L1, _lib.NORM_L2_MASS) == (6, 3, 4)
    assert (pamg.ERROR, pamg.NORM_L1, pamg.NORM_L2_MASS) == (6, 3, 4)
    count = int(re.search(r"#define\s+PAMG_K_COUNT\s+(\d+)", text).group(1))
    assert count == len(_lib.K_NAMES) == 19
    L = _lib.lib()
    assert hasattr(L, "pamg_get_error") and hasattr(L, "pamg_error_norm")
    assert hasattr(pamg.SemiImplicitIterative, "get_error") and hasattr(pamg.SemiImplicitIterative, "error_norm")


@pytest.mark.parametrize("mesh,S,L,levels", SHAPES, ids=IDS)
def test_oracle_m12_is_the_area_over_12(mesh, S, L, levels):
    """CPU: M_12 of the oracle's stencil against A_un / 4**i_split / 12 (exact), in ulp of M_12: at most 8, so the
    L2_MASS bound needs no addition (measured maximum over these shapes: 1.98 ulp, 900_ele S2)"""
    m = O.read_msh(path_of(mesh))
    o = O.Oracle(m, S, L)
    area = areas(m.X)
    worst = 0.0
    for l in range(1, L + 1):
        M = o.geometry(l)[1]
        for u in range(m.U):
            m12 = float(M[0, 1, u])
            ulps = abs(Fraction(m12) - area[u] / 12 / 4 ** (S - l + 1)) / Fraction(float(np.spacing(m12)))
            worst = max(worst, float(ulps))
    print("max |M_12 - A/12/4**i| in ulp:", worst)
    assert worst <= 8.0


# ---------------------------------------------------------------- 2. against the reference's own output
@gpu
@pytest.mark.parametrize("name", ["vtu_u8_s2_l2", "vtu_irregular_s3_l3"])
def test_error_field_matches_the_reference_vtu(name):
    """run as tests/test_vtu.py does; the device's error field to half a unit of the reference's F10.7"""
    import pamg
    z = np.load(os.path.join(goldens.GOLDEN, name + ".npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    s = pamg.SemiImplicitIterative(pamg.Mesh.read(path_of(meta["mesh"])), meta["n_split"], meta["levels"])
    s.run(meta["ntime"] - 1, meta["n_multigrid"])
    s.get_error()
    e = s.get(pamg.ERROR).reshape(-1, order="F")
    d = float(np.abs(e - z["error"]).max())
    print("max |error - fixture|:", d)
    assert d <= 5e-8 + 1e-16
    s.close()


# ---------------------------------------------------------------- 3. against numpy
@gpu
@pytest.mark.parametrize("mesh,S,L,levels", SHAPES, ids=IDS)
def test_error_field_against_numpy(mesh, S, L, levels):
    """|get(ERROR) - |tnew - sin(x + y)|| <= (3 R + 4) u (module docstring); zero before the first get_error;
    set(ERROR) refused"""
    import pamg
    s = solver((mesh, S, L))
    x, y = coords(s, (mesh, S))
    z = s.get(pamg.ERROR)
    assert z.shape == x.shape and not z.any()
    for kind in KINDS:
        assert s.field_norm(pamg.ERROR, 1, kind) == 0.0, kind
    t = np.random.default_rng(20261020).uniform(-1.0, 1.0, x.shape)
    s.set(pamg.TNEW, 1, t)
    assert not s.get(pamg.ERROR).any()   # setting tnew does not touch it
    s.get_error()
    e = s.get(pamg.ERROR)
    d = float(np.abs(e - np.abs(t - np.sin(x + y))).max())
    print("max difference: %.3e, bound %.3e" % (d, field_bound(x, y)))
    assert d <= field_bound(x, y)
    assert (e >= 0.0).all()
    with pytest.raises(pamg.PamgError) as err:
        s.set(pamg.ERROR, 1, e)
    assert err.value.rc == -1
    np.testing.assert_array_equal(s.get(pamg.ERROR), e)
    np.testing.assert_array_equal(s.get(pamg.TNEW, 1), t)
    if L > 1:   # level 1 only
        with pytest.raises(pamg.PamgError) as err:
            s.get(pamg.ERROR, 2)
        assert err.value.rc == -1
        with pytest.raises(pamg.PamgError) as err:
            s.field_norm(pamg.ERROR, 2, pamg.NORM_MAXABS)
        assert err.value.rc == -1
    s.close()


# ---------------------------------------------------------------- 4. planted deviations
@gpu
@pytest.mark.parametrize("mesh,S,L,levels", SHAPES, ids=IDS)
def test_planted_deviation_is_found(mesh, S, L, levels):
    """tnew = sin(x + y) + 0.5 at one entry: the first, the last, the last of each component, the first of the
    second un_ele and, on levels of at most 128 sub-elements, every entry (every storage position, up and down)"""
    import pamg
    s = solver((mesh, S, L))
    x, y = coords(s, (mesh, S))
    base = np.sin(x + y)
    bound = field_bound(x, y)
    nsub, Uloc = s.nsub(1), s.U
    spots = planted_spots(nsub, Uloc)
    if nsub * Uloc <= 128:
        spots += [np.unravel_index(i, base.shape, order="F") for i in range(base.size)]
    worst = 0.0
    for spot in spots:
        t = base.copy()
        t[spot] += 0.5
        s.set(pamg.TNEW, 1, t)
        v = s.error_norm(pamg.NORM_MAXABS)
        worst = max(worst, abs(v - 0.5))
        assert abs(v - 0.5) <= bound, (spot, v)
        assert s.error_norm(pamg.NORM_REF) == v, spot   # the field is non-negative
        s.get_error()
        e = s.get(pamg.ERROR)
        assert np.unravel_index(int(np.argmax(e)), e.shape) == tuple(int(q) for q in spot), spot
        assert e[spot] == v
        e[spot] = 0.0
        assert float(e.max()) <= bound, spot
    print("max |MAXABS - 0.5|: %.3e, bound %.3e" % (worst, bound))
    s.close()


# ---------------------------------------------------------------- 5. fused equals stored, bitwise
@gpu
@pytest.mark.parametrize("mesh,S,L,levels", SHAPES, ids=IDS)
def test_error_norm_is_get_error_then_field_norm(mesh, S, L, levels):
    import pamg
    s = solver((mesh, S, L))
    rng = np.random.default_rng(7)
    for trial in range(2):
        if trial == 0:
            s.set(pamg.TNEW, 1, rng.uniform(-1.0, 1.0, (3, s.nsub(1), s.U)))
        else:   # a computed state
            s.begin_timestep()
            s.vcycle(2)
        fused = [s.error_norm(k) for k in KINDS]   # before the field exists / is current
        s.get_error()
        stored = [s.field_norm(pamg.ERROR, 1, k) for k in KINDS]
        assert fused == stored, (trial, fused, stored)
        assert [s.error_norm(k) for k in KINDS] == stored
        e = s.get(pamg.ERROR)
        ref, mx, ss = expected(e)
        assert fused[pamg.NORM_REF] == ref and fused[pamg.NORM_MAXABS] == mx and ref == mx
        assert_l2(fused[pamg.NORM_L2], ss, e.size, "L2")
        assert_l1(fused[pamg.NORM_L1], e, "L1")
    s.close()


# ---------------------------------------------------------------- 6. the new kinds on plain fields
@gpu
@pytest.mark.parametrize("mesh,S,L,levels", SHAPES, ids=IDS)
def test_l1_and_l2_mass_on_plain_fields(mesh, S, L, levels):
    import pamg
    s = solver((mesh, S, L))
    area = areas(s.mesh.X)
    rng = np.random.default_rng(20261021)
    for l in levels:
        nsub, Uloc = s.nsub(l), s.U
        a = rng.uniform(-1.0, 1.0, (3, nsub, Uloc))
        s.set(pamg.RESIDUAL, l, a)
        assert_l1(s.field_norm(pamg.RESIDUAL, l, pamg.NORM_L1), a, f"L{l} L1")
        assert_mass(s.field_norm(pamg.RESIDUAL, l, pamg.NORM_L2_MASS), mass_sq_exact(a, area, S - l + 1),
                    nsub * Uloc, f"L{l} L2_MASS")
        # a deviation in one sub-element's component moves the value as its own mass says (wrong weights show)
        for spot in planted_spots(nsub, Uloc):
            b = a.copy()
            b[spot] = 3.0
            s.set(pamg.RESIDUAL, l, b)
            assert_l1(s.field_norm(pamg.RESIDUAL, l, pamg.NORM_L1), b, f"L{l} L1 {spot}")
            assert_mass(s.field_norm(pamg.RESIDUAL, l, pamg.NORM_L2_MASS), mass_sq_exact(b, area, S - l + 1),
                        nsub * Uloc, f"L{l} L2_MASS {spot}")
        # the existing kinds are what they were
        s.set(pamg.RESIDUAL, l, a)
        ref, mx, ss = expected(a)
        assert s.field_norm(pamg.RESIDUAL, l, pamg.NORM_REF) == ref
        assert s.field_norm(pamg.RESIDUAL, l, pamg.NORM_MAXABS) == mx
        assert_l2(s.field_norm(pamg.RESIDUAL, l, pamg.NORM_L2), ss, a.size, f"L{l} L2")
        np.testing.assert_array_equal(s.get(pamg.RESIDUAL, l), a)
    # v == 1 on level 1: the squared value is the mesh area
    one = np.ones((3, s.nsub(1), s.U))
    s.set(pamg.TNEW, 1, one)
    assert_mass(s.field_norm(pamg.TNEW, 1, pamg.NORM_L2_MASS), sum(area, Fraction(0)), s.nsub(1) * s.U, "area")
    assert s.field_norm(pamg.TNEW, 1, pamg.NORM_L1) == float(one.size)
    s.close()


@gpu
def test_new_kinds_are_refused_by_the_residual_forms():
    import pamg
    s = solver(U8_33)
    s.begin_timestep()
    before = full_state(s)
    for kind in (pamg.NORM_L1, pamg.NORM_L2_MASS):
        for call in (lambda: s.residual_norm(1, kind), lambda: s.solve(1e-3, 4, kind=kind)):
            with pytest.raises(pamg.PamgError) as e:
                call()
            assert e.value.rc == -1
    for call in (lambda: s.error_norm(5), lambda: s.error_norm(-1), lambda: s.field_norm(pamg.TNEW, 1, 5)):
        with pytest.raises(pamg.PamgError) as e:
            call()
        assert e.value.rc == -1
    assert_states_equal(full_state(s), before, "a refused call changed the state")
    s.close()


# ---------------------------------------------------------------- 7. read-only
@gpu
@pytest.mark.parametrize("kw", [dict(), dict(op=1, monitor=1)], ids=["op0", "op1-monitor"])
def test_error_norm_is_read_only_and_get_error_writes_only_the_error(kw):
    import pamg
    a, c = solver(U8_33, **kw), solver(U8_33, **kw)
    for x in (a, c):
        x.begin_timestep()
        x.vcycle(2)
    before = full_state(a)
    vals = [a.error_norm(k) for k in KINDS]
    assert all(math.isfinite(v) and v > 0.0 for v in vals), vals
    assert_states_equal(full_state(a), before, "after error_norm")
    a.vcycle(2)
    c.vcycle(2)
    assert_states_equal(full_state(a), full_state(c), "after error_norm and two more cycles")
    before = full_state(a)
    a.get_error()
    assert_states_equal(full_state(a), before, "after get_error")
    assert a.get(pamg.ERROR).any()
    a.vcycle(2)
    c.vcycle(2)
    assert_states_equal(full_state(a), full_state(c), "after get_error and two more cycles")
    a.close()
    c.close()


# ---------------------------------------------------------------- 8. non-finite
@gpu
def test_non_finite_tnew_gives_nan_for_every_kind():
    import pamg
    s = solver(U8_33)
    rng = np.random.default_rng(3)
    base = rng.uniform(-1.0, 1.0, (3, s.nsub(1), s.U))
    for spot in ((0, 0, 0), (2, s.nsub(1) - 1, s.U - 1), (1, 37, 4)):
        for bad in (np.nan, np.inf, -np.inf):
            t = base.copy()
            t[spot] = bad
            s.set(pamg.TNEW, 1, t)
            s.get_error()
            for kind in KINDS:
                assert math.isnan(s.error_norm(kind)), (spot, bad, kind)
                assert math.isnan(s.field_norm(pamg.ERROR, 1, kind)), (spot, bad, kind)
    s.set(pamg.TNEW, 1, base)
    assert all(math.isfinite(s.error_norm(k)) for k in KINDS)
    s.close()


# ---------------------------------------------------------------- 9. partitions
@gpu
@pytest.mark.parametrize("nparts", [2, 4])
def test_partitioned_error_norms_are_the_single_domains(nparts):
    import pamg
    from pamg.solver import local_group, run_ranks
    mesh, S, L = U8_33
    m = pamg.Mesh.read(path_of(mesh))
    full = pamg.SemiImplicitIterative(m, S, L)
    t = np.random.default_rng(11).uniform(-1.0, 1.0, (3, full.nsub(1), m.U))
    full.set(pamg.TNEW, 1, t)
    ref = [full.error_norm(k) for k in KINDS]
    full.get_error()
    e = full.get(pamg.ERROR)
    n, n_sub = e.size, full.nsub(1) * m.U
    exact_mass = mass_sq_exact(e, areas(m.X), S)
    _, _, ss = expected(e)
    assert_l1(ref[pamg.NORM_L1], e, "single domain L1")
    assert_l2(ref[pamg.NORM_L2], ss, n, "single domain L2")
    assert_mass(ref[pamg.NORM_L2_MASS], exact_mass, n_sub, "single domain L2_MASS")

    owner = m.x_strip_owner(nparts)
    parts = [pamg.SemiImplicitIterative(m, S, L, comm=(nparts, r, None, owner)) for r in range(nparts)]
    for r, p in enumerate(parts):
        p.set(pamg.TNEW, 1, t[:, :, np.flatnonzero(owner == r)])
    local_group(parts)
    outs = {id(p): {} for p in parts}

    def drive(p):
        out = outs[id(p)]
        out["fused"] = [p.error_norm(k) for k in KINDS]
        p.get_error()
        out["stored"] = [p.field_norm(pamg.ERROR, 1, k) for k in KINDS]

    run_ranks(parts, drive)
    first = outs[id(parts[0])]
    for r, p in enumerate(parts):
        out = outs[id(p)]
        assert out["fused"] == out["stored"], r
        assert out["fused"] == first["fused"], "every rank receives the same double"
        v = out["fused"]
        assert v[pamg.NORM_REF] == ref[pamg.NORM_REF] and v[pamg.NORM_MAXABS] == ref[pamg.NORM_MAXABS], r
        assert_l1(v[pamg.NORM_L1], e, f"rank {r} L1")
        assert_l2(v[pamg.NORM_L2], ss, n, f"rank {r} L2")
        got = Fraction(v[pamg.NORM_L2_MASS]) ** 2
        assert abs(got - exact_mass) <= Fraction(n) * Fraction(U) * exact_mass, (r, float(got), float(exact_mass))
        np.testing.assert_array_equal(p.get(pamg.ERROR), e[:, :, np.flatnonzero(owner == r)], err_msg=f"rank {r}")
        p.close()
    full.close()


@gpu
def test_detached_partition_returns_its_local_error_norms():
    import pamg
    mesh, S, L = U8_33
    m = pamg.Mesh.read(path_of(mesh))
    owner = m.x_strip_owner(2)
    own = np.flatnonzero(owner == 1)
    p = pamg.SemiImplicitIterative(m, S, L, comm=(2, 1, None, owner))
    t = np.random.default_rng(5).uniform(-1.0, 1.0, (3, p.nsub(1), p.U))
    p.set(pamg.TNEW, 1, t)
    v = [p.error_norm(k) for k in KINDS]
    p.get_error()
    e = p.get(pamg.ERROR)
    assert v == [p.field_norm(pamg.ERROR, 1, k) for k in KINDS]
    ref, mx, ss = expected(e)
    assert v[pamg.NORM_REF] == ref and v[pamg.NORM_MAXABS] == mx
    assert_l1(v[pamg.NORM_L1], e, "detached L1")
    assert_l2(v[pamg.NORM_L2], ss, e.size, "detached L2")
    area = areas(m.X)
    assert_mass(v[pamg.NORM_L2_MASS], mass_sq_exact(e, [area[g] for g in own], S), p.nsub(1) * p.U, "detached L2_MASS")
    # and the values are the single domain's on these un_eles
    full = pamg.SemiImplicitIterative(m, S, L)
    tf = np.zeros((3, full.nsub(1), m.U))
    tf[:, :, own] = t
    full.set(pamg.TNEW, 1, tf)
    full.get_error()
    np.testing.assert_array_equal(full.get(pamg.ERROR)[:, :, own], e)
    full.close()
    p.close()


# ---------------------------------------------------------------- 10. the Fortran host
def _run_host(tmp_path, extra):
    shutil.copy(path_of("untitled8.msh"), tmp_path)
    (tmp_path / "pamg_run.nml").write_text(
        "&transport mesh_file='untitled8.msh', n_split=3, multi_levels=3, n_smooth=4, solver=3, ntime=2,\n"
        f" n_multigrid=2, device=0, call_sites=0{extra} /\n")
    r = subprocess.run([EXE], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@gpu
@pytest.mark.skipif(not os.access(EXE, os.X_OK), reason="the Fortran host is not built")
def test_fortran_host_reports_the_error_norms(tmp_path):
    import pamg
    s = solver(U8_33)
    s.run(2, 2)
    want = [s.error_norm(k) for k in (pamg.NORM_MAXABS, pamg.NORM_L2, pamg.NORM_L2_MASS)]
    s.close()
    (tmp_path / "on").mkdir()
    (tmp_path / "off").mkdir()
    on = _run_host(tmp_path / "on", ", report_error=1")
    off = _run_host(tmp_path / "off", "")
    lines = [ln for ln in on.splitlines() if ln.split()[:1] == ["error"]]
    assert len(lines) == 1, on
    got = [float(w) for w in lines[0].split()[1:]]
    assert got == want, (got, want)
    # without the switch the output is the parent's: no such line, and nothing else differs (the wall time aside)
    mask = lambda text: [re.sub(r"(cpu_time for time_loop =)\s*\S+", r"\1", ln)  # noqa: E731
                         for ln in text.splitlines()]
    assert not [ln for ln in off.splitlines() if ln.split()[:1] == ["error"]]
    assert mask(off) == [ln for ln in mask(on) if ln.split()[:1] != ["error"]]
