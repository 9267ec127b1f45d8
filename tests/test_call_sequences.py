"""Random public-call sequences against the oracle, bit for bit (tests/call_sequences.py).

The guard of libpamg's host-side bookkeeping: every listed (configuration, seed) is a program of about 25 public
calls -- the per-call routines, V-cycle calls, pamg_run, state uploads, schedule switches, the read-only norm calls
and one or two refused calls -- applied to a handle and to the oracle in lock-step, the whole state compared after
every call. The flavours and shapes are those tests/test_parameters.py names (the smallest that reach each
kernel); half the seeds run parameter set P1, the rest the defaults.

The seeds were picked with the oracle alone (test_listed_seeds_are_admissible): counting up from 1 or 2, the first
three per configuration whose program keeps every field finite with max|field| <= 1e6 after every operation.
"""
import numpy as np
import pytest

import call_sequences as Q
from test_parameters import IRR_42, U8_33, U8_53, U8_63

gpu = pytest.mark.gpu
E900_22, IRR_43 = ("900_ele.msh", 2, 2), ("irregular.msh", 4, 3)

CONFIGS = (
    # op 0, cycle 0, Gauss-Seidel: per-step, the two fused launches (one and two streams), pipelined / resident
    [Q.config(s, fused=f, arith=a) for s in (U8_33, U8_53, U8_63) for f in (0, 1, 2, 3) for a in (0, 1)] +
    # Richardson: fused only in the resident call
    [Q.config(s, solver=2, fused=f) for s in (U8_33, IRR_42) for f in (3, 0)] +
    # the corrected cycle: the resident call and the per-step path
    [Q.config(s, cycle=1, solver=sv, fused=f) for s in (U8_33, U8_53) for sv in (1, 3) for f in (3, 0)] +
    # the direct coarse solve
    [Q.config(s, coarse_solver=1, cycle=c) for s in (U8_33, E900_22) for c in (0, 1)] +
    # the face operator with its monitor image
    [Q.config(s, op=1, monitor=1, cycle=c, solver=sv) for s in (U8_33, IRR_43, U8_53) for c in (0, 1)
     for sv in (1, 3)] +
    # two x-strips through the multi-rank exchange path
    [Q.config(U8_33, parts=2, op=0), Q.config(U8_33, parts=2, op=1, monitor=1)]
)
# the default seeds are (1, 2, 3) and (2, 3, 4) in turn, so that half of all runs use P1 (the even seeds); listed
# here are the configurations where a default seed's program was inadmissible on the oracle (Richardson does not
# converge at the default dt: most of its admissible programs are P1's)
SEEDS = {
    "untitled8-S3-L3-fused3-solver2": (1, 2, 4),
    "untitled8-S3-L3-fused0-solver2": (2, 4, 6),
    "irregular-S4-L2-fused3-solver2": (2, 4, 6),
    "irregular-S4-L2-fused0-solver2": (2, 4, 6),
}
CASES = [(cfg, seed) for i, cfg in enumerate(CONFIGS)
         for seed in SEEDS.get(Q.config_id(cfg), (1 + i % 2, 2 + i % 2, 3 + i % 2))]
IDS = [f"{Q.config_id(cfg)}-seed{seed}" for cfg, seed in CASES]


# ---------------------------------------------------------------- CPU
def test_generator_is_deterministic_for_a_seed():
    for cfg in (CONFIGS[0], CONFIGS[-1]):
        assert Q.generate(cfg, 7) == Q.generate(cfg, 7)
        assert Q.generate(cfg, 7) != Q.generate(cfg, 8)
    text = Q.format_program(Q.generate(CONFIGS[0], 7))
    assert len(text.splitlines()) == len(Q.generate(CONFIGS[0], 7))   # one line per operation


def test_the_configuration_ids_are_unique_and_half_the_seeds_run_p1():
    assert len(set(IDS)) == len(IDS)
    p1 = sum(Q.param_set(seed) == "P1" for _, seed in CASES)
    assert abs(2 * p1 - len(CASES)) <= len(CASES) // 3 + 1, (p1, len(CASES))


@pytest.mark.parametrize("cfg,seed", CASES, ids=IDS)
def test_programs_meet_the_weighting_guarantees(cfg, seed):
    """a set directly before a vcycle, a per-call routine and a read-only call between two vcycle calls; the two
    uploads the caches depend on, one or two refused calls, about 25 operations, only legal levels otherwise"""
    prog = Q.generate(cfg, seed)
    assert Q.guarantees(prog) == (True, True, True), Q.format_program(prog)
    L = cfg["shape"][2]
    pairs = list(zip(prog, prog[1:]))
    assert any(a[:2] == ("set", "RESIDUAL") and b[0] == "vcycle" and b[1] >= 1 for a, b in pairs)
    assert any(a[:3] == ("set", "TNEW", L) and b[0] == "vcycle" and b[1] >= 1 for a, b in pairs)
    assert 1 <= sum(op[0] == "illegal" for op in prog) <= 2
    assert any(a[0] == "smoother" and a[1] >= 2 and b == ("vcycle", 0) for a, b in pairs)
    assert 20 <= len(prog) <= 34, len(prog)
    ctx = Q.Ctx(cfg)
    assert prog[0] == ("begin_timestep",) or ctx.solver == 2
    for op, nxt in zip(prog, prog[1:] + [None]):
        if op[0] == "illegal":
            continue
        if op[0] in Q.PER_CALL + ("residual_norm", "get_convergence"):
            assert 1 <= op[1] <= L - (op[0] == "prolongator"), op
        if op[0] == "smoother":
            assert op[1] == ctx.tnn and 1 <= op[2] <= 3, op
        if op[0] == "set" and op[2] == 1 and op[1] in ("TOLD", "RHS") and ctx.solver != 2:
            assert nxt == ("begin_timestep",), op
        if op == ("direct_solve", 1) or op[:3] == ("field_norm", "RHS", 1):
            assert not Q.excluded("read RHS_L1", ctx), op
        if op[0] == "set_call_schedule":
            assert ctx.schedule_ok, op
        if op[0] in ("residual_norm", "solve"):
            assert ctx.residual_norm_ok, op
        ctx.advance(op)


_ADMITTED = {}


@pytest.mark.parametrize("cfg,seed", CASES, ids=IDS)
def test_listed_seeds_are_admissible(cfg, seed):
    """on the oracle alone every field is finite with max|field| <= 1e6 after every operation (the goldens'
    admission rule with room for the uniform(-1, 1) uploads). The oracle does not depend on fused, monitor or
    the partition, so flavours that differ only there share a run when their programs are the same."""
    prog = Q.generate(cfg, seed)
    key = (cfg["shape"], tuple((k, v) for k, v in cfg["kw"].items() if k not in ("fused", "monitor")), seed,
           tuple(op for op in prog if op[0] != "set_call_schedule"))
    if key not in _ADMITTED:
        _ADMITTED[key] = Q.run_model(cfg, seed, prog)
    ok, at = _ADMITTED[key]
    assert ok, f"inadmissible at operation {at}:\n{Q.format_program(prog, (at or 0) + 1)}"


def test_exclusion_table_is_what_the_header_documents():
    """every entry of the table cites a consequence (a) .. (d) that include/pamg.h spells out, and there are no
    more entries than the header's paragraph backs (one may cite a consequence twice)"""
    import os
    import re
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pamg.h")) as f:
        text = " ".join(f.read().split())
    start = text.index("Level 1's right-hand side")
    para = text[start:text.index("*/", start)]
    documented = set(re.findall(r"\(([a-d])\)", para))
    assert documented == {"a", "b", "c", "d"}
    cited = [re.match(r"\(([a-d])\)", reason).group(1) for _, _, reason in Q.EXCLUSIONS]
    assert set(cited) == documented and len(Q.EXCLUSIONS) <= len(documented) + 1


def test_clone_is_deep_and_read_only_models_leave_the_oracle_alone():
    cfg = Q.config(U8_33, op=1)
    o = Q.make_oracle(cfg, 2)
    o.begin_timestep()
    o.vcycle()
    before = Q.model_state(o)
    c = o.clone()
    for k, v in Q.model_state(c).items():
        np.testing.assert_array_equal(v, before[k], err_msg=k)
    c.begin_timestep()
    c.vcycle()
    c.set(0, 2, np.ones((3, c.nsub(2), c.mesh.U)))
    r = Q.model_residual(o, 1)
    assert np.isfinite(r).all() and r.any()
    for k, v in Q.model_state(o).items():
        np.testing.assert_array_equal(v, before[k], err_msg=k)
    o2 = Q.make_oracle(cfg, 2)   # the clone went on as the original would have
    for _ in range(2):
        o2.begin_timestep()
        o2.vcycle()
    np.testing.assert_array_equal(c.get(0, 1), o2.get(0, 1))


# ---------------------------------------------------------------- GPU
@gpu
@pytest.mark.parametrize("cfg,seed", CASES, ids=IDS)
def test_call_sequence_is_bitwise_the_oracle(cfg, seed):
    Q.run_gpu(cfg, seed)
