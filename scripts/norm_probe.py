"""The convergence monitor at the bench shape (untitled8192, n_split 5, 3 levels, level 1; GPU box only).

(a) kernel time of the read-only residual reduction (timing class norm: k_residual_reduce + its combine
    launch) against get_residual's k_residual (timing class residual) on the same handle in the same
    process: 50 launches each, one event pair per launch, the median; repeated three times. k_residual is
    the yardstick: the norm moves 2/3 of its bytes and must not be slower, the margin being the largest
    difference among the residual's own three medians.
(b) the cost of a check: wall time of solve(tol = -1, max_cycles = 200, check_every = k) less that of the
    same 200 cycles in vcycle(k) calls, per check, for k = 1, 5, 20 and, to find where the checks fall under
    5 % of the cycles' time, 50 and 100 (median of three runs each).

--op 1: the face operator's leg (op = 1, monitor = 1, bench.py's face configuration: Gauss-Seidel, 4 sweeps).
(a) the read-only check residual_norm(1) -- the monitor words launch, k_face_residual_reduce and the combine --
    against the stored path on the same handle in the same process: get_residual(1) (the words refresh plus
    k_face<3>) followed by field_norm(RESIDUAL). Both end with the read-back of one record, so each is timed
    as the wall time of its calls, 50 of each, the median; repeated three times. The read-only check must not
    be slower than the pair, the margin being the largest difference among the pair's own three medians. The
    device time of the timing classes is printed beside it (the stored path's words refresh belongs to no
    timing class, so its device figure leaves that launch out).
(b) as above, for check_every = 1, 5, 20, relative to one op = 1 cycle.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "p-a_multigrids_amd"))
import pamg  # noqa: E402
from pamg._lib import K_NAMES  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--op", type=int, default=0, choices=(0, 1))
OP = ap.parse_args().op
LAUNCHES, REPS, CYCLES, HBM = 50, 3, 200, 8e12

mesh = pamg.Mesh.read(os.path.join(ROOT, "tests", "meshes", "untitled8192.msh"))
if OP == 1:
    s = pamg.SemiImplicitIterative(mesh, 5, 3, n_smooth=4, solver=3, op=1, monitor=1)
else:
    s = pamg.SemiImplicitIterative(mesh, 5, 3, n_smooth=4, solver=3, arith=1, fused=3)
s.begin_timestep()
s.vcycle(40 if OP == 0 else 10)
s.synchronize()
N = s.nsub(1) * s.U
print(f"norm_probe: untitled8192 n_split 5, 3 levels, level 1, op = {OP}: N = {N} sub-elements, U = {s.U}")


def one(name, call):
    """the kernel time (ms) and algorithmic bytes of one launch of timing class `name`"""
    s.timing_reset()
    call()
    k = s.timing()[name]
    assert k["launches"] == 1, (name, k)
    return k["ms"], k["bytes"]


def face_leg():
    """(a) of the --op 1 leg"""
    def check():
        s.residual_norm(1, pamg.NORM_MAXABS)

    def stored():
        s.get_residual(1)
        s.field_norm(pamg.RESIDUAL, 1, pamg.NORM_MAXABS)

    def timed(call):
        """(wall s, {class: (ms, bytes)}) of one call"""
        s.timing_reset()
        t0 = time.perf_counter()
        call()
        t = time.perf_counter() - t0
        tm = s.timing()
        return t, {n: (tm[n]["ms"], tm[n]["bytes"]) for n in ("norm", "residual")}

    s.timing_enable(1 << K_NAMES.index("norm") | 1 << K_NAMES.index("residual"))
    s.timing_stride(1)
    for _ in range(5):
        check()
        stored()
    med = {"check": [], "stored": []}
    for rep in range(REPS):
        for name, call in (("check", check), ("stored", stored)):
            v = [timed(call) for _ in range(LAUNCHES)]
            w = float(np.median([x[0] for x in v]))
            dev = float(np.median([x[1]["norm"][0] + x[1]["residual"][0] for x in v])) * 1e-3
            by = v[0][1]["norm"][1] + v[0][1]["residual"][1]
            med[name].append(w)
            print(f"(a) rep {rep}: {name:6s} median of {LAUNCHES}: wall {w * 1e6:8.2f} us; timed launches "
                  f"{dev * 1e6:8.2f} us, {by / 1e6:.1f} MB algorithmic, {by / dev / 1e12:.2f} TB/s "
                  f"({100 * by / dev / HBM:.1f} % of 8 TB/s)")
    margin = max(med["stored"]) - min(med["stored"])
    worst = max(med["check"]) - min(med["stored"])
    print(f"(a) stored-path medians {['%.2f' % (x * 1e6) for x in med['stored']]} us, margin (their largest "
          f"difference) {margin * 1e6:.2f} us; read-only check medians {['%.2f' % (x * 1e6) for x in med['check']]} us")
    print(f"(a) slowest check median - fastest stored-path median = {worst * 1e6:+.2f} us: "
          f"{'not slower' if worst <= margin else 'SLOWER'} than get_residual + field_norm within the margin")
    s.timing_enable(0)


def block_leg():
    """(a) of the op = 0 leg"""
    s.timing_enable(1 << K_NAMES.index("norm") | 1 << K_NAMES.index("residual"))
    s.timing_stride(1)
    for _ in range(5):   # warm both kernels
        s.residual_norm(1, pamg.NORM_MAXABS)
        s.get_residual(1)
    med = {"norm": [], "residual": []}
    for rep in range(REPS):
        for name, call in (("norm", lambda: s.residual_norm(1, pamg.NORM_MAXABS)),
                           ("residual", lambda: s.get_residual(1))):
            v = [one(name, call) for _ in range(LAUNCHES)]
            ms = float(np.median([x[0] for x in v]))
            med[name].append(ms)
            print(f"(a) rep {rep}: {name:8s} median of {LAUNCHES} launches {ms * 1e3:8.2f} us, "
                  f"{v[0][1] / 1e6:.1f} MB algorithmic, {v[0][1] / (ms * 1e-3) / 1e12:.2f} TB/s "
                  f"({100 * v[0][1] / (ms * 1e-3) / HBM:.1f} % of 8 TB/s)")
    margin = max(med["residual"]) - min(med["residual"])
    worst = max(med["norm"]) - min(med["residual"])
    print(f"(a) residual medians {['%.2f' % (x * 1e3) for x in med['residual']]} us, margin (their largest "
          f"difference) {margin * 1e3:.2f} us; norm medians {['%.2f' % (x * 1e3) for x in med['norm']]} us")
    print(f"(a) slowest norm median - fastest residual median = {worst * 1e3:+.2f} us: "
          f"{'not slower' if worst <= margin else 'SLOWER'} than k_residual within the margin")
    s.timing_enable(0)


if OP == 1:
    face_leg()
    CYCLES = 100   # an op = 1 cycle takes several times an op = 0 one
else:
    block_leg()


def wall(fn):
    v = []
    for _ in range(3):
        s.begin_timestep()
        s.synchronize()
        t0 = time.perf_counter()
        fn()
        s.synchronize()
        v.append(time.perf_counter() - t0)
    return float(np.median(v))


under = None
for k in ((1, 5, 20, 50, 100) if OP == 0 else (1, 5, 20)):
    def plain():
        for _ in range(CYCLES // k):
            s.vcycle(k)
    t_plain = wall(plain)
    t_solve = wall(lambda: s.solve(-1.0, CYCLES, check_every=k))
    checks = CYCLES // k
    per = (t_solve - t_plain) / checks
    frac = (t_solve - t_plain) / t_plain
    if under is None and frac < 0.05:
        under = k
    print(f"(b) check_every {k:2d}: {CYCLES} cycles in vcycle({k}) calls {t_plain * 1e3:8.3f} ms, solve "
          f"{t_solve * 1e3:8.3f} ms, {checks} checks: {per * 1e6:7.1f} us per check, "
          f"{100 * frac:.1f} % of the cycles' time, {per / (t_plain / CYCLES):.3f} of one cycle")
print("(b) the checks fall under 5 % of the cycles' time at check_every = " +
      (str(under) if under is not None else "none of those measured"))
s.close()
