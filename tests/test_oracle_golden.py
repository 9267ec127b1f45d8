"""Pin the C oracle (oracle/pamg_oracle.c) against the reference's own outputs.

The golden vectors in tests/golden were produced by compiling and running the
reference Fortran (oracle/build_ref.py + tests/make_golden.py). Each fp64
case must match to 1e-12 relative (observed: bit-exact); the as-shipped fp32
build is only within ~1e-5 of fp64, which is checked
as a property of the reference, not of the oracle.
"""
import os

import numpy as np
import pytest

import goldens
import oracle_lib as O

TOL = 1e-12
STATE_KEYS = ("tnew", "told", "RHS", "res")


def make_oracle(meta, **kw):
    mesh = O.read_msh(os.path.join(goldens.MESHES, meta["mesh"]))
    return mesh, O.Oracle(mesh, meta["n_split"], meta["levels"], n_smooth=meta["n_smooth"],
                          solver=meta["solver"], ntime=meta["ntime"], n_multigrid=meta["n_multigrid"],
                          **goldens.physics(meta), **kw)


FP64 = [n for n in goldens.names() if not n.endswith("fp32")]


@pytest.mark.parametrize("name", FP64)
def test_topology_matches_reference(name):
    meta, d = goldens.load(name)
    mesh = O.read_msh(os.path.join(goldens.MESHES, meta["mesh"]))
    U = mesh.U
    assert d["Neig"].shape == (3, U)
    np.testing.assert_array_equal(mesh.neig.reshape((3, U), order="F"), d["Neig"])
    np.testing.assert_array_equal(mesh.fneig.reshape((3, U), order="F"), d["fNeig"])
    np.testing.assert_array_equal(mesh.dir.reshape((3, U), order="F"), d["Dir"])
    np.testing.assert_array_equal(mesh.region, d["region"][0])
    np.testing.assert_array_equal(mesh.X.reshape((2, 3, U), order="F"), d["X"])


@pytest.mark.parametrize("name", [n for n in FP64 if "8192" not in n])
def test_geometry_matches_reference(name):
    meta, d = goldens.load(name)
    _, o = make_oracle(meta)
    for l in range(1, meta["levels"] + 1):
        dw, M, Kd, ml = o.geometry(l)
        assert goldens.rel_err(dw, d[f"detwei_L{l}"]) <= TOL
        assert goldens.rel_err(M, d[f"mass_L{l}"]) <= TOL
        assert goldens.rel_err(Kd, d[f"kdiff_L{l}"]) <= TOL
        assert goldens.rel_err(ml, d[f"ml_L{l}"]) <= TOL


@pytest.mark.parametrize("name", FP64)
def test_final_state_matches_reference(name):
    meta, d = goldens.load(name)
    _, o = make_oracle(meta)
    o.run()
    st = o.state()
    tov, tovo = o.overlap()
    st["t_overlap"], st["t_overlap_old"] = tov, tovo
    for k, v in st.items():
        if k in d:
            assert goldens.rel_err(v, d[k]) <= TOL, (k, goldens.rel_err(v, d[k]))
        else:
            assert goldens.compare_sampled(d, k, v) <= TOL, k


def _replay_first_cycle(o, meta, d):
    """Drive the oracle through the first V-cycle call by call, in the order of
    transport_tri_semi.F90:319-379, checking against each reference dump."""
    L = meta["levels"]
    tags = goldens.calls(d)
    seq = []
    for l in range(1, L + 1):
        seq += [("copy", l), ("smooth", l), ("restrict", l), ("residual", l)]
    seq += [("copy", L), ("coarse", L)]
    for l in range(L - 1, 0, -1):
        seq += [("copy", l), ("prolong", l), ("smooth", l)]
    o.begin_timestep()
    it = iter(tags)
    checked = 0
    for op, l in seq:
        if op == "copy":
            o.copy_to_tnn(l)
            continue
        if op == "smooth":
            o.smoother(l)
        elif op == "restrict":
            o.restrictor(l)
        elif op == "residual":
            o.get_residual(l)
        elif op == "coarse":
            for _ in range(meta.get("n_coarse", 15)):
                o.smoother(l)
        elif op == "prolong":
            o.prolongator(l)
        tag = next(it)
        assert tag.endswith(f"{op}_L{l}"), (tag, op, l)
        st = o.state()
        for k, v in st.items():
            ref = d[f"{tag}/{k}"]
            assert goldens.rel_err(v, ref) <= TOL, (tag, k, goldens.rel_err(v, ref))
        checked += 1
    assert checked == len(tags)


@pytest.mark.parametrize("name", [n for n in FP64 if any("/" in k for k in goldens.load(n)[1])])
def test_each_call_of_first_vcycle_matches_reference(name):
    meta, d = goldens.load(name)
    _, o = make_oracle(meta)
    _replay_first_cycle(o, meta, d)


def test_fp32_reference_is_within_1e4_of_fp64():
    """Property of the reference itself: as-shipped default-real arithmetic
    deviates from the fp64-promoted build at the 1e-5 level."""
    _, d32 = goldens.load("u8_s3_l3_gs_fp32")
    _, d64 = goldens.load("u8_s3_l3_gs")
    e = goldens.rel_err(d32["tnew_L1"], d64["tnew_L1"])
    assert 0 < e < 1e-4


def test_quirk_jacobi_equals_gauss_seidel():
    """with the block-diagonal operator solver=1 and solver=3 coincide."""
    _, dj = goldens.load("u8_s3_l3_jacobi")
    _, dg = goldens.load("u8_s3_l3_gs")
    for k in ("tnew_L1", "tnew_L2", "tnew_L3", "res_L1", "tnew_nonlin"):
        np.testing.assert_array_equal(dj[k], dg[k])


def test_quirk_single_sweep_never_moves_fine_level():
    """n_smooth=1 keeps only the pre-sweep iterate in tnew."""
    _, d = goldens.load("u8_s2_l2_smooth1")
    assert np.all(d["tnew_L1"] == 0.0)
    assert np.any(d["tnew_nonlin"] != 0.0)


def test_quirk_coarse_levels_do_not_feed_fine_level():
    """the prolonged correction is overwritten, so the fine
    solution does not depend on the number of levels once L >= 2 (L = 1 makes
    level 1 the coarse level, which receives the 15 extra smoother calls)."""
    mesh = O.read_msh(os.path.join(goldens.MESHES, "untitled8.msh"))
    outs = []
    for L in (2, 3):
        o = O.Oracle(mesh, 3, L)
        o.run()
        outs.append(o.get(O.TNEW, 1))
    np.testing.assert_array_equal(outs[0], outs[1])
