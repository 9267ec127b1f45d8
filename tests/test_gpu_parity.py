"""GPU parity of the HIP path (libpamg through its C-ABI) against the reference.

Every comparison is against the reference's own fp64 outputs (tests/golden,
produced by compiling and running the reference) or against the C oracle
pinned to them (tests/test_oracle_golden.py). Tolerance: 1e-10 relative to the
array's max magnitude (the north star's bar); the kernels reproduce the
reference's operation order without FMA contraction, so the observed errors
are ~1e-16 (only the device sine of the level-1 source term differs).
"""
import os

import numpy as np
import pytest

import goldens
import oracle_lib as O
import pamg
from pamg.solver import halo_loopback

pytestmark = pytest.mark.gpu
TOL = 1e-10
FP64 = [n for n in goldens.names() if not n.endswith("fp32")]


def gpu_solver(meta, **kw):
    mesh = pamg.Mesh.read(os.path.join(goldens.MESHES, meta["mesh"]))
    args = dict(n_smooth=meta["n_smooth"], solver=meta["solver"], **goldens.physics(meta))
    args.update(kw)
    return pamg.SemiImplicitIterative(mesh, meta["n_split"], meta["levels"], **args)


def compare(st, d, tag=""):
    worst = 0.0
    for k, v in st.items():
        key = f"{tag}/{k}" if tag else k
        if key in d:
            e = goldens.rel_err(v, d[key])
        else:
            e = goldens.compare_sampled(d, key, v)
        assert e <= TOL, (key, e)
        worst = max(worst, e)
    return worst


@pytest.mark.parametrize("name", FP64)
def test_time_loop_matches_reference(name):
    meta, d = goldens.load(name)
    s = gpu_solver(meta)
    s.run(meta["ntime"], meta["n_multigrid"])
    st = s.state()
    st["t_overlap"], st["t_overlap_old"] = s.overlap()
    compare(st, d)


@pytest.mark.parametrize("name", [n for n in FP64 if any("/" in k for k in goldens.load(n)[1])])
def test_each_reference_call_site(name):
    """Drive the fine-grained C-ABI call by call in the order of
    transport_tri_semi.F90:319-379 and compare after every call."""
    meta, d = goldens.load(name)
    s = gpu_solver(meta)
    L = meta["levels"]
    seq = []
    for l in range(1, L + 1):
        seq += [("copy", l), ("smooth", l), ("restrict", l), ("residual", l)]
    seq += [("copy", L), ("coarse", L)]
    for l in range(L - 1, 0, -1):
        seq += [("copy", l), ("prolong", l), ("smooth", l)]
    s.begin_timestep()
    tags = iter(goldens.calls(d))
    for op, l in seq:
        if op == "copy":
            s.copy_to_tnn(l)
            continue
        {"smooth": lambda: s.smoother(l), "restrict": lambda: s.restrictor(l),
         "residual": lambda: s.get_residual(l), "coarse": lambda: s.smoother(l, meta.get("n_coarse", 15)),
         "prolong": lambda: s.prolongator(l)}[op]()
        tag = next(tags)
        assert tag.endswith(f"{op}_L{l}")
        compare(s.state(), d, tag)


def test_driver_equals_fine_grained_calls_bitwise():
    meta, _ = goldens.load("u8_s3_l3_gs")
    a = gpu_solver(meta)
    a.run(2, 2)
    b = gpu_solver(meta)
    L = meta["levels"]
    for _ in range(2):
        b.begin_timestep()
        for _ in range(2):
            for l in range(1, L + 1):
                b.copy_to_tnn(l); b.smoother(l); b.restrictor(l); b.get_residual(l)
            b.copy_to_tnn(L); b.smoother(L, 15)
            for l in range(L - 1, 0, -1):
                b.copy_to_tnn(l); b.prolongator(l); b.smoother(l)
    sa, sb = a.state(), b.state()
    for k in sa:
        np.testing.assert_array_equal(sa[k], sb[k], err_msg=k)
    np.testing.assert_array_equal(a.overlap()[0], b.overlap()[0])


def test_per_sweep_halo_mode_is_state_identical():
    """the per-step kernels: the halo written once per smoother call (halo_mode 0) or before
    every sweep (1, one launch per sweep) leave the same state"""
    meta, _ = goldens.load("irregular_s3_l3")
    a = gpu_solver(meta, halo_mode=0, fused=0)
    b = gpu_solver(meta, halo_mode=1, fused=0)
    a.run(2, 2)
    b.run(2, 2)
    for k, v in a.state().items():
        np.testing.assert_array_equal(v, b.state()[k], err_msg=k)
    for x, y in zip(a.overlap(), b.overlap()):
        np.testing.assert_array_equal(x, y)


def test_jacobi_equals_gauss_seidel_on_gpu():
    meta, _ = goldens.load("u8_s3_l3_gs")
    a = gpu_solver(meta, solver=1)
    b = gpu_solver(meta, solver=3)
    a.run(2, 2)
    b.run(2, 2)
    for k, v in a.state().items():
        np.testing.assert_array_equal(v, b.state()[k], err_msg=k)


@pytest.mark.parametrize("mesh,S,L", [("untitled8192.msh", 5, 3), ("irregular.msh", 6, 3), ("900_ele.msh", 4, 4)])
def test_full_size_against_oracle(mesh, S, L):
    """BASELINE sizes: untitled8192 at n_split=5 (8.4 M fine sub-elements),
    irregular.msh at n_split=6 (config 5, P1); one time step, one V-cycle."""
    m = pamg.Mesh.read(os.path.join(goldens.MESHES, mesh))
    s = pamg.SemiImplicitIterative(m, S, L)
    s.run(1, 1)
    om = O.read_msh(os.path.join(goldens.MESHES, mesh))
    o = O.Oracle(om, S, L, ntime=1, n_multigrid=1)
    o.run()
    so, sg = o.state(), s.state()
    for k in so:
        assert goldens.rel_err(sg[k], so[k]) <= TOL, k
    for x, y in zip(s.overlap(), o.overlap()):
        assert goldens.rel_err(x, y) <= TOL


@pytest.mark.parametrize("S,nparts,fused,exch", [(3, 2, 3, 0), (3, 2, 3, 1), (3, 2, 1, 0), (3, 2, 0, 0),
                                                 (5, 8, 3, 0), (5, 8, 1, 1)])
def test_partitioned_run_matches_single_gpu(S, nparts, fused, exch):
    """Partitions of untitled8192 (x-strips) on one GPU, halo exchanged by the loopback
    path (the same packed segments RCCL carries between ranks); exch = 0 packs the
    exchange once per pamg_vcycle call, 1 after every cycle. n_split = 5 in 8 parts is
    the 8-GPU bench's per-rank launch (1,024 workgroups: the 64-VGPR instance)."""
    mesh = pamg.Mesh.read(os.path.join(goldens.MESHES, "untitled8192.msh"))
    full = pamg.SemiImplicitIterative(mesh, S, 3)
    full.run(1, 3)
    owner = mesh.x_strip_owner(nparts)
    parts = [pamg.SemiImplicitIterative(mesh, S, 3, comm=(nparts, r, None, owner), fused=fused,
                                        halo_exchange=exch) for r in range(nparts)]
    for p in parts:
        p.run(1, 3)
    halo_loopback(parts, 1)
    ref_state = full.state()
    ref_ov = full.overlap()
    for r, p in enumerate(parts):
        own = np.flatnonzero(owner == r)
        for k, v in p.state().items():
            np.testing.assert_array_equal(v, ref_state[k][:, :, own], err_msg=k)
        for x, y in zip(p.overlap(), ref_ov):
            np.testing.assert_array_equal(x, y[:, :, own])


def test_state_errors_are_reported():
    meta, _ = goldens.load("u8_s3_l3_gs")
    s = gpu_solver(meta)
    s.begin_timestep()
    with pytest.raises(pamg.PamgError):
        s.smoother(2)          # tnew_nonlin holds level 1
    with pytest.raises(pamg.PamgError):
        s.prolongator(3)       # no coarser level
    with pytest.raises(pamg.PamgError):
        s.get_residual(4)


def test_timing_counts_launches():
    meta, _ = goldens.load("u8_s3_l3_gs")
    s = gpu_solver(meta, fused=0)
    s.timing_enable(0xFF)
    s.timing_reset()
    s.run(1, 1)
    t = s.timing()
    assert t["smooth_L1"]["launches"] == 2 and t["smooth"]["launches"] == 4
    # the driver fuses restrictor(l) with the following get_residual(l) (:336, :338)
    assert t["residual"]["launches"] == 3 and t["restrict"]["launches"] == 0
    assert t["prolong"]["launches"] == 2 and t["rhs"]["launches"] == 1


def test_fused_vcycle_counts_one_launch_per_cycle():
    meta, _ = goldens.load("u8_s3_l3_gs")
    s = gpu_solver(meta, fused=1)
    s.timing_enable(0xF7F)
    s.timing_reset()
    s.run(2, 3)
    t = s.timing()
    assert t["vcycle"]["launches"] == 6 and t["vcycle_coarse"]["launches"] == 6
    assert t["smooth_L1"]["launches"] == 0 and t["prolong"]["launches"] == 0
    assert t["rhs"]["launches"] == 2


def test_pipelined_vcycle_launches():
    """fused = 3: a call of n cycles is coarse(1), n - 1 pipelined launches, level 1 (n); inside
    pamg_run a step's last launch is pipelined too, carrying the next step's first coarse
    cycle, so 2 steps of 3 cycles are coarse, 5 pipelined, level 1."""
    meta, _ = goldens.load("u8_s3_l3_gs")
    s = gpu_solver(meta, fused=3)
    s.set_call_schedule(1)
    s.timing_enable(0xF7F)
    s.timing_reset()
    s.vcycle(3)
    t = s.timing()
    assert t["vcycle_coarse"]["launches"] == 1 and t["vcycle_pipe"]["launches"] == 2
    assert t["vcycle"]["launches"] == 1
    s.timing_reset()
    s.run(2, 3)
    t = s.timing()
    # each step's first pipelined launch also starts the step (told, RHS: vcycle_rhsf)
    assert t["vcycle_coarse"]["launches"] == 1 and t["vcycle_rhsf"]["launches"] == 2
    assert t["vcycle_pipe"]["launches"] == 3 and t["rhs"]["launches"] == 0
    assert t["vcycle"]["launches"] == 1 and t["smooth_L1"]["launches"] == 0


def test_resident_vcycle_launches():
    """fused = 3, schedule 3 (automatic where it applies): a call of n cycles is one launch; a
    pamg_run of several steps is one launch that also starts every step (told, RHS:
    vcycle_res_rhsf)."""
    meta, _ = goldens.load("u8_s3_l3_gs")
    s = gpu_solver(meta, fused=3)
    s.timing_enable(0x3F7F)
    s.timing_reset()
    s.vcycle(3)
    t = s.timing()
    assert t["vcycle_res"]["launches"] == 1 and t["vcycle_coarse"]["launches"] == 0
    assert t["vcycle_pipe"]["launches"] == 0 and t["vcycle"]["launches"] == 0
    s.timing_reset()
    s.run(2, 3)
    t = s.timing()
    assert t["vcycle_res_rhsf"]["launches"] == 1 and t["vcycle_res"]["launches"] == 0
    assert t["rhs"]["launches"] == 0 and t["vcycle_pipe"]["launches"] == 0 and t["smooth_L1"]["launches"] == 0
    # one launch moves every level's state in and out once, whatever the number of cycles
    assert t["vcycle_res_rhsf"]["bytes"] > 0


def test_resident_run_is_one_launch():
    """Every resident configuration: a whole pamg_run (every time step: told := tnew, the RHS, n_multigrid
    cycles) is one resident launch; its state equals the step-by-step public calls bit for bit
    (test_time_loop_equals_public_steps, schedule 3)."""
    m = pamg.Mesh.read(os.path.join(goldens.MESHES, "untitled2048.msh"))
    s = pamg.SemiImplicitIterative(m, 5, 3, arith=1, fused=3)
    s.timing_enable(0x3F7F)
    s.timing_reset()
    s.run(4, 2)
    t = s.timing()
    assert t["vcycle_res_rhsf"]["launches"] == 1 and t["vcycle_res"]["launches"] == 0
    assert t["rhs"]["launches"] == 0 and t["vcycle_pipe"]["launches"] == 0
    s.close()


@pytest.mark.parametrize("mesh,S,L,solver,ns", [
    ("untitled8.msh", 1, 1, 3, 1), ("untitled8.msh", 2, 2, 3, 2), ("untitled8.msh", 3, 3, 1, 1),
    ("irregular.msh", 3, 3, 3, 1), ("900_ele.msh", 2, 2, 3, 3), ("900_ele.msh", 4, 4, 1, 1),
    ("untitled2048.msh", 5, 5, 3, 1), ("untitled8192.msh", 5, 3, 3, 4), ("test_sn2.msh", 4, 2, 3, 2),
    # n_split >= 6: a tile is a part of an un_ele (4 tiles at 6, 16 at 7)
    ("irregular.msh", 6, 3, 3, 4), ("irregular.msh", 7, 4, 1, 2), ("untitled2048.msh", 6, 3, 3, 4),
    ("900_ele.msh", 6, 5, 3, 1), ("test_sn2.msh", 7, 2, 3, 1),
    # n_split = 8: 64 tiles per un_ele, 256 positions along an un_ele face
    ("untitled8.msh", 8, 3, 3, 2), ("irregular.msh", 8, 5, 1, 1)])
@pytest.mark.parametrize("fused", [1, 2, 3])
def test_fused_vcycle_equals_kernel_sequence_bitwise(mesh, S, L, solver, ns, fused):
    """The one-launch V-cycle (pamg_vcycle.hip) computes the same operations in
    the same order as the per-step kernels: every field of every level and the
    halo arrays agree bit for bit, including partial tiles (U not a multiple of
    the tile's element count) and meshes with boundary faces. fused = 2 runs the
    coarse-level and level-1 launches of a cycle concurrently (double-buffered
    level-2 RHSN across three consecutive cycles); fused = 3 pipelines them (level 1 of
    cycle c with the coarse levels of cycle c + 1 in one launch)."""
    m = pamg.Mesh.read(os.path.join(goldens.MESHES, mesh))
    a = pamg.SemiImplicitIterative(m, S, L, n_smooth=ns, solver=solver, fused=fused)
    b = pamg.SemiImplicitIterative(m, S, L, n_smooth=ns, solver=solver, fused=0)
    a.run(2, 3)
    b.run(2, 3)
    sa, sb = a.state(), b.state()
    for k in sb:
        np.testing.assert_array_equal(sa[k], sb[k], err_msg=k)
    for x, y in zip(a.overlap(), b.overlap()):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("mesh,S,L", [("untitled2048.msh", 5, 3), ("irregular.msh", 6, 3), ("900_ele.msh", 3, 2)])
@pytest.mark.parametrize("fused", [1, 3])
def test_fused_vcycle_halo_mode1_bitwise(mesh, S, L, fused):
    """halo_mode = 1 (the reference's schedule: the halo rewritten before every sweep) runs the
    fused forms too, and leaves the state of the per-step kernels with halo_mode = 1 -- every
    field and t_overlap / t_overlap_old -- bit for bit (a time loop of 2 steps x 3 cycles)."""
    m = pamg.Mesh.read(os.path.join(goldens.MESHES, mesh))
    a = pamg.SemiImplicitIterative(m, S, L, fused=fused, halo_mode=1, arith=1)
    b = pamg.SemiImplicitIterative(m, S, L, fused=0, halo_mode=1, arith=1)
    a.timing_enable(0x3F7F)
    a.run(2, 3)
    b.run(2, 3)
    assert a.timing()["smooth_L1"]["launches"] == 0   # the fused path ran
    sa, sb = a.state(), b.state()
    for k in sb:
        np.testing.assert_array_equal(sa[k], sb[k], err_msg=k)
    for x, y in zip(a.overlap(), b.overlap()):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("mesh,S,L", [("irregular.msh", 4, 3), ("untitled2048.msh", 5, 3), ("900_ele.msh", 3, 2)])
@pytest.mark.parametrize("fused", [1, 2, 3])
def test_fused_vcycle_interleaved_with_call_sites_bitwise(mesh, S, L, fused):
    """Fused V-cycles mixed with the per-call entry points and state uploads: the fused path's
    cached restriction (RHSN) and once-per-step halo words must follow every other writer."""
    m = pamg.Mesh.read(os.path.join(goldens.MESHES, mesh))
    a = pamg.SemiImplicitIterative(m, S, L, fused=fused)
    b = pamg.SemiImplicitIterative(m, S, L, fused=0)
    rng = np.random.default_rng(20251015)
    res1 = rng.uniform(-1e-9, 1e-9, (3, a.nsub(1), a.U))
    told = rng.uniform(-1e-6, 1e-6, (3, a.nsub(1), a.U))
    for s in (a, b):
        s.begin_timestep()
        s.vcycle(1)
        s.copy_to_tnn(1)
        s.smoother(1)
        s.get_residual(2)
        s.vcycle(2)
        s.set(pamg.RESIDUAL, 1, res1)
        s.vcycle(1)
        s.set(pamg.TOLD, 1, told)
        s.vcycle(1)
        s.begin_timestep()
        s.vcycle(2)
    sa, sb = a.state(), b.state()
    for k in sb:
        np.testing.assert_array_equal(sa[k], sb[k], err_msg=k)
    for x, y in zip(a.overlap(), b.overlap()):
        np.testing.assert_array_equal(x, y)


# ---- contracted operator arithmetic (pamg_params.arith = 1): A_e = (1/dt) M + Kd assembled
# once per un_ele, one fma chain per row. Exact parity of that arithmetic is
# tests/test_contracted_oracle.py (bitwise against the oracle's restatement of it, the bench
# config included). Here it is held against the reference's operation order, whose roundings
# differ: the solution (level-1 tnew / tnew_nonlin / told / RHS and the halo arrays -- the north
# star's "solution vector") to 1e-12 relative, 100x inside its 1e-10 bar (observed ~1e-15). The
# residual-derived fields (res_l; RHS_l, tnew_l for l >= 2) are differences of nearly equal
# terms: an fp64 evaluation in ANY operation order, the reference's included, fixes them only to
# eps times the magnitude of the terms, which is the scale of the level-1 data they come from
# (RHS_{l+1} is the restriction of res_l = A x_l - RHS_l). They are held to 1e-12 of that
# scale -- max|RHS_1| for the RHS-unit fields (res, RHS), max|tnew_1| for the solution-unit
# ones (tnew) -- a bound that does not depend on how far the levels have converged (observed
# <= 2e-15 of it; on bench.py's workload every level is well conditioned, kappa_l =
# max|RHS_l| / max|res_l| <= 8, and the same numbers are <= 4e-13 of each level's own RHS scale:
# archive/profiles/r02_conditioning.txt). With arith = 0 every field is bitwise.
TOL_CONTRACTED = 1e-12
SOLUTION = ("tnew_L1", "told_L1", "RHS_L1", "tnew_nonlin", "t_overlap", "t_overlap_old")


def check_contracted(st, ref, levels, err_of):
    """err_of(k, v) -> max abs difference of field k from the reference's"""
    rhs1 = float(np.abs(ref("RHS_L1")).max())
    # the level-1 iterate's scale: tnew_L1, or the last sweep (tnew_nonlin) when tnew is still zero
    # (n_smooth = 1 keeps the fine tnew at exactly 0)
    t1 = max(float(np.abs(ref("tnew_L1")).max()),
             float(np.abs(ref("tnew_nonlin")).max()) if ref("tnew_nonlin") is not None else 0.0)
    for l in range(1, levels + 1):
        for k, scale in ((f"res_L{l}", rhs1),) + (((f"RHS_L{l}", rhs1), (f"tnew_L{l}", t1), (f"told_L{l}", t1))
                                                    if l >= 2 else ()):
            if k in st:
                e = err_of(k, st[k])
                assert e <= TOL_CONTRACTED * scale, (k, e, scale)
    for k in SOLUTION:
        if k in st:
            r = ref(k)
            e = err_of(k, st[k])
            assert e <= TOL_CONTRACTED * max(float(np.abs(r).max()), 1e-300), (k, e)


def golden_ref(d):
    def get(k):
        if k in d:
            return d[k]
        if k + "@sample" in d:
            return d[k + "@sample"]
        return None
    return get


@pytest.mark.parametrize("name", FP64)
def test_contracted_time_loop_matches_reference(name):
    meta, d = goldens.load(name)
    if meta["solver"] == 2:
        pytest.skip("Richardson has no operator product (arith applies to solver 1/3)")

    def err_of(k, v):   # max abs difference (sampled fields: on the stored sample)
        if k in d:
            return float(np.abs(np.asarray(v) - d[k]).max())
        return goldens.compare_sampled(d, k, v) * float(np.abs(golden_ref(d)(k)).max())

    for fused in (0, 1, 2, 3):
        s = gpu_solver(meta, arith=1, fused=fused)
        s.run(meta["ntime"], meta["n_multigrid"])
        st = s.state()
        st["t_overlap"], st["t_overlap_old"] = s.overlap()
        check_contracted(st, golden_ref(d), meta["levels"], err_of)


@pytest.mark.parametrize("mesh,S,L", [("untitled8192.msh", 5, 3), ("irregular.msh", 6, 3), ("900_ele.msh", 3, 3),
                                      ("untitled2048.msh", 6, 3), ("irregular.msh", 7, 4)])
def test_contracted_full_size_against_oracle(mesh, S, L):
    """BASELINE sizes, one time step of two V-cycles, the pipelined fused schedule."""
    m = pamg.Mesh.read(os.path.join(goldens.MESHES, mesh))
    s = pamg.SemiImplicitIterative(m, S, L, arith=1, fused=3)
    s.run(1, 2)
    om = O.read_msh(os.path.join(goldens.MESHES, mesh))
    o = O.Oracle(om, S, L, ntime=1, n_multigrid=2)
    o.run()
    so, sg = o.state(), s.state()
    so["t_overlap"], so["t_overlap_old"] = o.overlap()
    sg["t_overlap"], sg["t_overlap_old"] = s.overlap()
    check_contracted(sg, so.get, L, lambda k, v: float(np.abs(np.asarray(v) - so[k]).max()))


@pytest.mark.parametrize("mesh,S,L,ns", [("untitled8.msh", 3, 3, 1), ("irregular.msh", 3, 3, 4),
                                         ("900_ele.msh", 4, 4, 2), ("untitled2048.msh", 5, 5, 3),
                                         ("irregular.msh", 6, 3, 4), ("untitled2048.msh", 6, 4, 2),
                                         ("irregular.msh", 7, 5, 1), ("untitled8.msh", 8, 4, 2)])
@pytest.mark.parametrize("fused", [1, 2, 3])
def test_contracted_fused_equals_kernel_sequence_bitwise(mesh, S, L, ns, fused):
    m = pamg.Mesh.read(os.path.join(goldens.MESHES, mesh))
    a = pamg.SemiImplicitIterative(m, S, L, n_smooth=ns, arith=1, fused=fused)
    b = pamg.SemiImplicitIterative(m, S, L, n_smooth=ns, arith=1, fused=0)
    a.run(2, 3)
    b.run(2, 3)
    sa, sb = a.state(), b.state()
    for k in sb:
        np.testing.assert_array_equal(sa[k], sb[k], err_msg=k)
    for x, y in zip(a.overlap(), b.overlap()):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("mesh,S,L", [("untitled8192.msh", 5, 3), ("irregular.msh", 4, 4), ("900_ele.msh", 3, 2),
                                      ("irregular.msh", 6, 3)])
@pytest.mark.parametrize("arith", [0, 1])
def test_pipelined_call_boundaries_are_invisible(mesh, S, L, arith):
    """fused = 3 pipelines the cycles of one pamg_vcycle call (coarse levels one cycle ahead
    inside the call): one call of 5 cycles, five calls of one, and calls of 2 + 3 leave the
    same state, bit for bit."""
    m = pamg.Mesh.read(os.path.join(goldens.MESHES, mesh))
    runs = []
    for split in ([5], [1] * 5, [2, 3]):
        s = pamg.SemiImplicitIterative(m, S, L, arith=arith, fused=3)
        s.begin_timestep()
        for n in split:
            s.vcycle(n)
        st = s.state()
        st["t_overlap"], st["t_overlap_old"] = s.overlap()
        runs.append(st)
    for st in runs[1:]:
        for k in runs[0]:
            np.testing.assert_array_equal(st[k], runs[0][k], err_msg=k)


@pytest.mark.parametrize("mesh,S,L,n", [("untitled8192.msh", 5, 3, 5), ("untitled8192.msh", 3, 3, 2),
                                        ("irregular.msh", 4, 4, 3), ("900_ele.msh", 3, 2, 4),
                                        ("untitled8192.msh", 5, 4, 4), ("untitled2048.msh", 5, 5, 3)])
@pytest.mark.parametrize("arith", [0, 1])
def test_call_schedules_equal_one_sequence(mesh, S, L, n, arith):
    """Pipelined calls as two tile halves on two streams (schedule 2) and resident calls (every
    cycle of the call in one launch, schedule 3) leave the state of one launch per cycle, bit
    for bit, t_overlap included."""
    m = pamg.Mesh.read(os.path.join(goldens.MESHES, mesh))
    runs = []
    for ts in (1, 2, 3):
        s = pamg.SemiImplicitIterative(m, S, L, arith=arith, fused=3)
        s.set_call_schedule(ts)
        s.begin_timestep()
        s.vcycle(n)
        s.vcycle(1)
        st = s.state()
        st["t_overlap"], st["t_overlap_old"] = s.overlap()
        runs.append(st)
        s.close()
    for r in runs[1:]:
        for k in runs[0]:
            np.testing.assert_array_equal(r[k], runs[0][k], err_msg=k)


@pytest.mark.parametrize("mesh,S,L,n", [("untitled8192.msh", 5, 3, 2), ("irregular.msh", 4, 4, 3),
                                        ("900_ele.msh", 3, 2, 1), ("untitled2048.msh", 5, 5, 2),
                                        ("irregular.msh", 6, 3, 2), ("irregular.msh", 7, 3, 1),
                                        ("untitled2048.msh", 5, 2, 2), ("untitled8192.msh", 3, 3, 2)])
@pytest.mark.parametrize("schedule", [1, 2, 3])
def test_time_loop_equals_public_steps(mesh, S, L, n, schedule):
    """pamg_run skips what a step leaves that the next step overwrites unread (the step-start
    tnew_nonlin copy, the last cycle's residual / tnew_nonlin / coarse RHS and residual / halo
    words and their exchange): its state after 3 steps equals 3 x (begin_timestep; vcycle),
    bit for bit, t_overlap included."""
    m = pamg.Mesh.read(os.path.join(goldens.MESHES, mesh))
    a = pamg.SemiImplicitIterative(m, S, L, arith=1, fused=3)
    b = pamg.SemiImplicitIterative(m, S, L, arith=1, fused=3)
    for s in (a, b):
        s.set_call_schedule(schedule)
    a.run(3, n)
    for _ in range(3):
        b.begin_timestep()
        b.vcycle(n)
    sa, sb = a.state(), b.state()
    for k in sb:
        np.testing.assert_array_equal(sa[k], sb[k], err_msg=k)
    for x, y in zip(a.overlap(), b.overlap()):
        np.testing.assert_array_equal(x, y)
    a.close()
    b.close()


@pytest.mark.parametrize("S,nparts", [(3, 2), (5, 8)])
def test_partitioned_time_loop_matches_single_gpu(S, nparts):
    """Several time steps on partitions (pamg_run skips the exchanges of all but the last
    step) leave the single-domain state after the loopback exchange, bit for bit."""
    mesh = pamg.Mesh.read(os.path.join(goldens.MESHES, "untitled8192.msh"))
    full = pamg.SemiImplicitIterative(mesh, S, 3)
    full.run(3, 2)
    owner = mesh.x_strip_owner(nparts)
    parts = [pamg.SemiImplicitIterative(mesh, S, 3, comm=(nparts, r, None, owner), fused=3)
             for r in range(nparts)]
    for p in parts:
        p.run(3, 2)
    halo_loopback(parts, 1)
    ref_state = full.state()
    ref_ov = full.overlap()
    for r, p in enumerate(parts):
        own = np.flatnonzero(owner == r)
        for k, v in p.state().items():
            np.testing.assert_array_equal(v, ref_state[k][:, :, own], err_msg=k)
        for x, y in zip(p.overlap(), ref_ov):
            np.testing.assert_array_equal(x, y[:, :, own])


@pytest.mark.parametrize("mesh,S,L", [("untitled8.msh", 3, 3), ("irregular.msh", 6, 4), ("900_ele.msh", 2, 2)])
def test_state_round_trip_through_the_storage_order(mesh, S, L):
    """set_state / get_state convert between the reference's (3, nsub, U) row-wise numbering and
    the hierarchical storage order (Level::pos): every field of every level round-trips exactly,
    and the fused cycle started from uploaded state equals the per-step kernels' (both read it
    through the same permutation)."""
    m = pamg.Mesh.read(os.path.join(goldens.MESHES, mesh))
    rng = np.random.default_rng(20251015)
    a = pamg.SemiImplicitIterative(m, S, L, fused=3, arith=1)
    b = pamg.SemiImplicitIterative(m, S, L, fused=0, arith=1)
    for l in range(1, L + 1):
        for what in (pamg.TNEW, pamg.TOLD, pamg.RHS, pamg.RESIDUAL):
            v = rng.uniform(-1, 1, (3, a.nsub(l), a.U))
            for s in (a, b):
                s.set(what, l, v)
                np.testing.assert_array_equal(s.get(what, l), v)
    for s in (a, b):
        s.vcycle(3)
    sa, sb = a.state(), b.state()
    for k in sb:
        np.testing.assert_array_equal(sa[k], sb[k], err_msg=k)


@pytest.mark.parametrize("mesh,S,L,ns", [("untitled8.msh", 2, 2, 4), ("irregular.msh", 3, 3, 2), ("900_ele.msh", 4, 4, 1),
                                         ("untitled2048.msh", 5, 3, 4), ("irregular.msh", 6, 3, 3),
                                         ("test_sn2.msh", 7, 2, 2)])
def test_richardson_resident_equals_kernel_sequence_bitwise(mesh, S, L, ns):
    """solver = 2 (solve_Richardson, transport_tri_semi.F90:511-518) in the resident call: the update
    x + omega b and get_residual's rebuild of level 1's RHS from told (:865-867) after the step's
    first smoother call. A whole pamg_run is one resident launch, the public step sequence one per
    call; both equal the per-step kernels bit for bit, t_overlap included."""
    m = pamg.Mesh.read(os.path.join(goldens.MESHES, mesh))
    ref = pamg.SemiImplicitIterative(m, S, L, n_smooth=ns, solver=2, fused=0)
    ref.run(3, 2)
    run = pamg.SemiImplicitIterative(m, S, L, n_smooth=ns, solver=2, fused=3)
    run.timing_enable(0x3F7F)
    run.timing_reset()
    run.run(3, 2)
    t = run.timing()
    assert t["vcycle_res_rhsf"]["launches"] == 1 and t["smooth_L1"]["launches"] == 0
    steps = pamg.SemiImplicitIterative(m, S, L, n_smooth=ns, solver=2, fused=3)
    for _ in range(3):
        steps.begin_timestep()
        steps.vcycle(1)
        steps.vcycle(1)
    sr = ref.state()
    for s in (run, steps):
        st = s.state()
        for k in sr:
            np.testing.assert_array_equal(st[k], sr[k], err_msg=k)
        for x, y in zip(s.overlap(), ref.overlap()):
            np.testing.assert_array_equal(x, y)
