"""get_error on the device at the bench shape (untitled8192, n_split 5, 3 levels, level 1; GPU box only).

Kernel time through the timing class norm, one event pair per span, 50 calls of each route, the median; repeated
three times, on the same handle in the same process:
  fused   error_norm(NORM_L2): k_error_reduce + the combine launch (24 B per sub-element in, nothing out)
  stored  get_error() + field_norm(ERROR, 1, NORM_L2): k_error (24 B in, 24 B out), then k_field_reduce + the
          combine launch (24 B in) -- two spans, summed
  floor   field_norm(TNEW, 1, NORM_L2): k_field_reduce + the combine launch, the pure traffic of the fused pass
          without its three sines per sub-element
The fused call must not be slower than the stored route, the margin being the largest difference among that
route's own three medians.
"""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "p-a_multigrids_amd"))
import pamg  # noqa: E402
from pamg._lib import K_NAMES  # noqa: E402

LAUNCHES, REPS, HBM = 50, 3, 8e12

mesh = pamg.Mesh.read(os.path.join(ROOT, "tests", "meshes", "untitled8192.msh"))
s = pamg.SemiImplicitIterative(mesh, 5, 3, n_smooth=4, solver=3, arith=1, fused=3)
s.begin_timestep()
s.vcycle(40)
s.synchronize()
N = s.nsub(1) * s.U
print(f"error_probe: untitled8192 n_split 5, 3 levels, level 1: N = {N} sub-elements ({3 * N} nodes, 3 sines per "
      f"sub-element), U = {s.U}")


def fused():
    return s.error_norm(pamg.NORM_L2)


def stored():
    s.get_error()
    return s.field_norm(pamg.ERROR, 1, pamg.NORM_L2)


def floor():
    return s.field_norm(pamg.TNEW, 1, pamg.NORM_L2)


ROUTES = (("fused", fused, 1), ("stored", stored, 2), ("floor", floor, 1))


def one(call, spans):
    """(kernel ms, algorithmic bytes) of the norm-class spans of one call"""
    s.timing_reset()
    call()
    k = s.timing()["norm"]
    assert k["launches"] == spans, k
    return k["ms"], k["bytes"]


s.timing_enable(1 << K_NAMES.index("norm"))
s.timing_stride(1)
for _ in range(5):   # warm the kernels; the first stored() allocates the error field
    for _, call, _ in ROUTES:
        call()
assert fused() == stored(), "error_norm and get_error + field_norm disagree"
med = {name: [] for name, _, _ in ROUTES}
for rep in range(REPS):
    for name, call, spans in ROUTES:
        v = [one(call, spans) for _ in range(LAUNCHES)]
        ms = float(np.median([x[0] for x in v]))
        by = v[0][1]
        med[name].append(ms)
        print(f"rep {rep}: {name:6s} median of {LAUNCHES} calls {ms * 1e3:8.2f} us, {by / 1e6:.1f} MB algorithmic, "
              f"{by / (ms * 1e-3) / 1e12:.2f} TB/s ({100 * by / (ms * 1e-3) / HBM:.1f} % of 8 TB/s), "
              f"{3 * N / (ms * 1e-3) / 1e9:.1f} G nodes/s")
margin = max(med["stored"]) - min(med["stored"])
worst = max(med["fused"]) - min(med["stored"])
print(f"stored-route medians {['%.2f' % (x * 1e3) for x in med['stored']]} us, margin (their largest difference) "
      f"{margin * 1e3:.2f} us; fused medians {['%.2f' % (x * 1e3) for x in med['fused']]} us; floor medians "
      f"{['%.2f' % (x * 1e3) for x in med['floor']]} us")
print(f"slowest fused median - fastest stored-route median = {worst * 1e3:+.2f} us: "
      f"{'not slower' if worst <= margin else 'SLOWER'} than get_error + field_norm within the margin")
f, fl = float(np.median(med["fused"])), float(np.median(med["floor"]))
print(f"fused / floor = {f / fl:.2f}: the fused pass is "
      f"{'at the traffic floor (HBM-bound)' if f <= 1.15 * fl else 'above the traffic floor: bound by the fp64 sines, not by HBM'}")
s.timing_enable(0)
s.close()
