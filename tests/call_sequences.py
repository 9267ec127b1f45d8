"""Random sequences of public calls, driven against the oracle in lock-step.

The host side of libpamg keeps flags (rhsn_valid, overlap_static_l1, told_halo_stale_l1, rhs_pending, tnn_level,
xe_ev_valid) and cached copies (the fused cycle's restriction RHSN, the compact told copy of the halo, the
double-buffered send words, the op = 1 replica of the coarsest tnew, the monitor halo image). Every public entry
point that writes a field must invalidate the right subset, and a miss shows only when calls are mixed in an order
nobody wrote down. The oracle (oracle/pamg_oracle.c) has no caches at all, so it is the model: a seeded generator
makes programs of about 25 public calls, and the driver applies each to a handle (or to the handles of a partition)
and to an Oracle, comparing the whole state after every call, bit for bit.

A program is a plain list of tuples and prints one operation per line (format_program); a failure carries the
seed, the configuration, the index of the failing operation and the program up to it, so that

    cfg, prog = <pasted>
    import call_sequences as Q
    Q.run_gpu(cfg, seed, program=prog)

replays it. Nothing here needs a GPU until run_gpu is called.
"""
import math
from fractions import Fraction

import numpy as np

import oracle_lib as O
from test_parameters import SETS, path_of

# ---------------------------------------------------------------------------------------------------------------
# The only comparisons and calls that may be left out: (operation, condition, reason). Each entry restates one
# consequence, (a) .. (d), of the paragraph "Level 1's right-hand side" in include/pamg.h; the generator and the
# driver consult this table through excluded() and nothing else skips anything. None applies to solver 2, whose
# right-hand side both sides assemble in get_residual(1) only.
EXCLUSIONS = (
    ("compare RHS_L1", "rhs1_pending",
     "(a) the library assembles level 1's RHS in pamg_begin_timestep, the reference (and the oracle) inside the "
     "next level-1 sweep or residual: between the two the oracle's array is the previous step's"),
    ("read RHS_L1", "rhs1_pending",
     "(b) for the same reason a call that reads level 1's RHS without sweeping level 1 -- direct_solve(1), "
     "field_norm(RHS, 1) -- has no model value in that window"),
    ("set TOLD_L1", "mid_step",
     "(c) told(1) written in mid-step never reaches the library's RHS, the oracle's next sweep assembles its "
     "RHS from it: generated only directly before a begin_timestep, which overwrites told"),
    ("set RHS_L1", "mid_step",
     "(d) RHS(1) written in mid-step stays in the library until the next pamg_begin_timestep, the oracle "
     "overwrites it in its next sweep: generated only directly before a begin_timestep"),
    ("level-1 work", "before_first_begin",
     "(a) again: before the first pamg_begin_timestep the library's level-1 RHS is still zero; every program "
     "starts with begin_timestep"),
)

FIELDS = {"TNEW": 0, "TOLD": 1, "RHS": 2, "RESIDUAL": 3, "TNEW_NONLIN": 4}
KIND_NAMES = ("REF", "MAXABS", "L2", "L1", "L2_MASS")
N_OPS = 25
ADMISSIBLE_MAX = 1e6


def excluded(what, ctx):
    """True when the table leaves `what` out in the state `ctx` (the one gate for every skipped comparison or call)"""
    if ctx.solver == 2:
        return False
    for op, cond, _ in EXCLUSIONS:
        if op == what:
            return {"rhs1_pending": ctx.rhs1_pending, "mid_step": True,
                    "before_first_begin": not ctx.begun}[cond]
    raise KeyError(what)


# ---------------------------------------------------------------------------------------------------------------
# configurations
def config(shape, parts=1, **kw):
    """a handle flavour: shape (mesh, n_split, levels), the pamg_params that differ from the defaults, the number
    of x-strips (1: a single domain)"""
    return dict(shape=tuple(shape), parts=parts, kw=dict(sorted(kw.items())))


def config_id(cfg):
    mesh, S, L = cfg["shape"]
    tag = "-".join(f"{k}{v}" for k, v in cfg["kw"].items())
    return f"{mesh.split('.')[0]}-S{S}-L{L}-{tag}" + (f"-x{cfg['parts']}" if cfg["parts"] > 1 else "")


def param_set(seed):
    """P1 of tests/test_parameters.py for the even seeds, the defaults for the odd ones: k = 1 hides nothing"""
    return "P1" if seed % 2 == 0 else "default"


class Ctx:
    """what the generator and the driver know of a handle without asking it: the level tnew_nonlin holds, and
    whether level 1's RHS is comparable (EXCLUSIONS)"""

    def __init__(self, cfg):
        kw = cfg["kw"]
        self.L = cfg["shape"][2]
        self.solver = kw.get("solver", 3)
        self.op, self.cycle, self.fused = kw.get("op", 0), kw.get("cycle", 0), kw.get("fused", 3)
        self.monitor = kw.get("monitor", 0)
        self.agg = self.op == 1 and cfg["parts"] > 1   # the coarsest level is a replica: its norms are refused
        self.tnn = 1
        self.begun = False
        self.rhs1_pending = False

    @property
    def schedule_ok(self):
        return self.fused == 3 and self.op == 0 and self.cycle == 0

    @property
    def residual_norm_ok(self):   # include/pamg.h: solver 1 or 3; op = 1 needs monitor = 1
        return self.solver != 2 and (self.op == 0 or self.monitor == 1)

    def advance(self, op):
        name = op[0]
        if name == "begin_timestep":
            self.tnn, self.begun, self.rhs1_pending = 1, True, True
        elif name in ("copy_to_tnn", "direct_solve"):
            self.tnn = op[1]
        elif name == "smoother":
            if op[1] == 1:
                self.rhs1_pending = False
        elif name in ("get_residual", "get_convergence"):
            if op[1] == 1:
                self.rhs1_pending = False
        elif name == "vcycle":
            if op[1] > 0:
                self.tnn, self.rhs1_pending = 1, False
        elif name == "solve":
            if op[1] > 0:
                self.tnn, self.rhs1_pending = 1, False
        elif name == "run":
            if op[1] > 0:
                self.tnn, self.begun, self.rhs1_pending = 1, True, op[2] == 0
        elif name == "set" and op[1] == "TNEW_NONLIN":
            self.tnn = op[2]


# ---------------------------------------------------------------------------------------------------------------
# generator
PER_CALL = ("copy_to_tnn", "smoother", "restrictor", "get_residual", "prolongator", "direct_solve")


def _level(rng, ctx, lo=1, hi=None):
    return int(rng.integers(lo, (hi or ctx.L) + 1))


def _norm_levels(ctx):
    return list(range(1, ctx.L + (0 if ctx.agg else 1)))


def _gen_set(rng, ctx, what=None, level=None):
    """a legal upload; a list, since told(1) and RHS(1) come with the begin_timestep that must follow them"""
    what = what or str(rng.choice(list(FIELDS)))
    level = level or _level(rng, ctx)
    op = ("set", what, level, int(rng.integers(1, 2 ** 31 - 1)))
    if level == 1 and what in ("TOLD", "RHS") and excluded(f"set {what}_L1", ctx):
        return [op, ("begin_timestep",)]
    return [op]


def _gen_per_call(rng, ctx, name=None):
    name = name or str(rng.choice(PER_CALL, p=(0.15, 0.3, 0.12, 0.18, 0.13, 0.12)))
    if name == "smoother":   # on the level tnew_nonlin holds, or after the copy that puts it there
        level = ctx.tnn if rng.random() < 0.4 else _level(rng, ctx)
        pre = [] if level == ctx.tnn else [("copy_to_tnn", level)]
        return pre + [("smoother", level, int(rng.integers(1, 4)))]
    if name == "prolongator":
        return [("prolongator", _level(rng, ctx, 1, ctx.L - 1))]
    if name == "direct_solve":
        level = _level(rng, ctx)
        if level == 1 and excluded("read RHS_L1", ctx):
            level = _level(rng, ctx, 2)
        return [("direct_solve", level)]
    return [(name, _level(rng, ctx))]


def _gen_read_only(rng, ctx):
    """a call that must leave the compared state as it was (get_error writes the ERROR field only)"""
    names = ["field_norm", "field_norm", "error_norm", "get_error"] + (["residual_norm"] * 3 if ctx.residual_norm_ok else [])
    name = str(rng.choice(names))
    levels = _norm_levels(ctx)
    if name == "residual_norm":
        return [("residual_norm", int(rng.choice(levels)), int(rng.integers(0, 3)))]
    if name == "error_norm":
        return [("error_norm", int(rng.integers(0, 5)))]
    if name == "get_error":
        return [("get_error",)]
    for _ in range(16):
        what = str(rng.choice(list(FIELDS)))
        level = ctx.tnn if what == "TNEW_NONLIN" else int(rng.choice(levels))
        if level not in levels or (what == "RHS" and level == 1 and excluded("read RHS_L1", ctx)):
            continue
        return [("field_norm", what, level, int(rng.integers(0, 5)))]
    return [("error_norm", 1)]


def _gen_illegal(rng, ctx):
    """a call the header refuses: the handle must answer with an error and leave everything as it was"""
    kind = int(rng.integers(0, 3))
    if kind == 0 and ctx.L > 1:   # a smoother on a level tnew_nonlin does not hold
        level = int(rng.choice([l for l in range(1, ctx.L + 1) if l != ctx.tnn]))
        return [("illegal", ("smoother", level, 1))]
    if kind == 1:
        return [("illegal", ("prolongator", ctx.L))]
    name = str(rng.choice(("copy_to_tnn", "smoother", "restrictor", "get_residual", "prolongator", "direct_solve")))
    level = int(rng.choice((0, ctx.L + 1, -1)))
    return [("illegal", (name, level, 1) if name == "smoother" else (name, level))]


def _gen_single(rng, ctx):
    names = ["begin_timestep", "per_call", "vcycle", "run", "set", "read_only", "get_convergence", "solve", "schedule"]
    p = np.array([0.07, 0.30, 0.12, 0.05, 0.15, 0.13, 0.05, 0.05 if ctx.residual_norm_ok else 0.0,
                  0.08 if ctx.schedule_ok else 0.0])
    name = str(rng.choice(names, p=p / p.sum()))
    if name == "begin_timestep":
        return [("begin_timestep",)]
    if name == "per_call":
        return _gen_per_call(rng, ctx)
    if name == "vcycle":
        return [("vcycle", int(rng.integers(0, 4)))]
    if name == "run":
        return [("run", int(rng.integers(0, 3)), int(rng.integers(1, 3)))]
    if name == "set":
        return _gen_set(rng, ctx)
    if name == "read_only":
        return _gen_read_only(rng, ctx)
    if name == "get_convergence":
        return [("get_convergence", int(rng.choice(_norm_levels(ctx))))]
    if name == "solve":
        return [("solve", int(rng.integers(1, 4)), int(rng.integers(1, 3)), int(rng.integers(0, 3)))]
    return [("set_call_schedule", int(rng.integers(1, 4)))]


def _vc(rng):
    return ("vcycle", int(rng.integers(1, 4)))


def generate(cfg, seed, n_ops=N_OPS):
    """The program of (configuration, seed): begin_timestep (EXCLUSIONS; not for solver 2), then in a random order
      - set(RESIDUAL, l) directly before a vcycle (the fused cycle's cached restriction must follow it),
      - set(TNEW, L) directly before a vcycle (so must the replica of the coarsest level),
      - a smoother call between two vcycle calls, two times in three on a coarse level (it writes that level's
        halo words, which the next fused cycle must put back), perhaps with another per-call routine after it,
      - a read-only call between two vcycle calls,
      - vcycle(0) directly after a smoother call on a coarse level: no pass of the loop, so nothing may move (the
        fused forms once put level 1's constant halo words back, and the op = 1 forms set tnn_level to 1, before
        looking at the count),
      - one or two calls the header refuses,
      - single operations drawn from the whole vocabulary, until the program has about n_ops operations.
    Only calls the header allows are emitted (Ctx tracks the level of tnew_nonlin) and only those the EXCLUSIONS
    table does not leave out."""
    rng = np.random.default_rng(seed)
    ctx = Ctx(cfg)
    items = ["set_res", "set_tnew", "per_call", "read_only", "no_op"] + ["illegal"] * int(rng.integers(1, 3))
    prog = []
    if excluded("level-1 work", ctx):
        prog.append(("begin_timestep",))
        ctx.advance(prog[0])
    items += ["single"] * max(0, n_ops - len(prog) - 15 - (len(items) - 5))   # (the five motifs: about 15 operations)

    def emit(ops):
        for op in ops:
            prog.append(op)
            if op[0] != "illegal":
                ctx.advance(op)

    for i in rng.permutation(len(items)):
        item = items[i]
        if item == "set_res":
            emit(_gen_set(rng, ctx, "RESIDUAL") + [_vc(rng)])
        elif item == "set_tnew":
            emit(_gen_set(rng, ctx, "TNEW", ctx.L) + [_vc(rng)])
        elif item == "per_call":
            emit([_vc(rng)])
            level = 1 if rng.random() < 1.0 / 3 else _level(rng, ctx, 2)
            emit(([] if level == ctx.tnn else [("copy_to_tnn", level)]) + [("smoother", level, int(rng.integers(1, 4)))])
            if rng.random() < 0.5:
                emit(_gen_per_call(rng, ctx))
            emit([_vc(rng)])
        elif item == "read_only":
            emit([_vc(rng)])
            emit(_gen_read_only(rng, ctx))
            emit([_vc(rng)])
        elif item == "no_op":
            level = _level(rng, ctx, 2)
            emit(([] if level == ctx.tnn else [("copy_to_tnn", level)]) + [("smoother", level, int(rng.integers(1, 3)))])
            emit([("vcycle", 0)])
        elif item == "illegal":
            emit(_gen_illegal(rng, ctx))
        else:
            emit(_gen_single(rng, ctx))
    return prog


def format_program(prog, upto=None):
    return "\n".join(f"  {i:2d} {op!r}," for i, op in enumerate(prog[:upto]))


READ_ONLY = ("residual_norm", "field_norm", "error_norm", "get_error")


def guarantees(prog):
    """the three weighting guarantees as booleans: a set directly before a vcycle; a per-call routine, and a
    read-only call, with nothing but per-call routines / read-only calls around it between two vcycle calls"""
    names = [op[0] for op in prog]
    set_vc = any(a == "set" and b == "vcycle" for a, b in zip(names, names[1:]))

    def between(kinds):
        last_vc = None
        for i, n in enumerate(names):
            if n == "vcycle":
                if last_vc is not None and i > last_vc + 1 and all(m in kinds for m in names[last_vc + 1:i]):
                    return True
                last_vc = i
        return False
    return set_vc, between(PER_CALL), between(READ_ONLY)


# ---------------------------------------------------------------------------------------------------------------
# the model
def set_array(op, nsub, U):
    """the array of a ("set", what, level, s) operation: uniform(-1, 1) from its own seed, whole domain"""
    return np.random.default_rng(op[3]).uniform(-1.0, 1.0, (3, nsub, U))


def make_oracle(cfg, seed, source=None):
    mesh, S, L = cfg["shape"]
    kw = {k: v for k, v in cfg["kw"].items() if k in ("solver", "cycle", "coarse_solver", "op", "arith")}
    cycle = kw.pop("cycle", 0)
    o = O.Oracle(O.read_msh(path_of(mesh)), S, L, **SETS[param_set(seed)], **kw)
    o.cycle = cycle
    if source is not None:
        o.set_source(source)
    return o


def model_cycles(o, n):
    for _ in range(n):
        o.vcycle_corrected() if o.cycle else o.vcycle()


def model_residual(o, level):
    """the residual a read-only call reduces: orc_get_residual on a clone that is then thrown away"""
    c = o.clone()
    c.get_residual(level)
    return c.get(O.RES, level)


def apply_model(o, op):
    """apply a writing operation to the oracle; returns the model value of the calls that also return one"""
    name = op[0]
    if name == "begin_timestep":
        o.begin_timestep()
    elif name == "copy_to_tnn":
        o.copy_to_tnn(op[1])
    elif name == "smoother":
        for _ in range(op[2]):
            o.smoother(op[1])
    elif name in ("restrictor", "get_residual", "prolongator", "direct_solve"):
        getattr(o, name)(op[1])
    elif name == "vcycle":
        model_cycles(o, op[1])
    elif name == "run":
        for _ in range(op[1]):
            o.begin_timestep()
            model_cycles(o, op[2])
    elif name == "set":
        _, what, level, _ = op
        if what == "TNEW_NONLIN":
            o.copy_to_tnn(level)   # gives tnew_nonlin the level's shape; every word is then overwritten
        o.set(FIELDS[what], level, set_array(op, o.nsub(level), o.mesh.U))
    elif name == "get_convergence":
        o.get_residual(op[1])
        return o.get(O.RES, op[1])
    elif name == "solve":
        _, max_cycles, check_every, _ = op
        residuals, done = [], 0
        while done < max_cycles:
            n = min(check_every, max_cycles - done)
            model_cycles(o, n)
            done += n
            residuals.append(model_residual(o, 1))
        return residuals
    elif name not in ("set_call_schedule", "illegal") + READ_ONLY:
        raise ValueError(op)
    return None


def model_state(o):
    st = o.state()
    st["t_overlap"], st["t_overlap_old"] = o.overlap()
    st["tnn_level"] = o.tnn_level()
    return st


def admissible(st):
    return all(np.isfinite(v).all() and float(np.abs(v).max()) <= ADMISSIBLE_MAX for v in st.values()
               if isinstance(v, np.ndarray))


def run_model(cfg, seed, program=None):
    """the program on the oracle alone: (admissible after every operation, index of the first inadmissible one)"""
    prog = program or generate(cfg, seed)
    o = make_oracle(cfg, seed)
    for i, op in enumerate(prog):
        apply_model(o, op)
        if not admissible(model_state(o)):
            return False, i
    return True, None


# ---------------------------------------------------------------------------------------------------------------
# the lock-step driver
class Failure(AssertionError):
    pass


def _fail(cfg, seed, prog, i, why):
    raise Failure(f"{why}\nseed {seed}, parameter set {param_set(seed)}, configuration {cfg!r}\n"
                  f"operation {i}: {prog[i]!r}\nprogram up to it:\n{format_program(prog, i + 1)}")


class Target:
    """one handle, or the handles of a partition driven collectively (one host thread per rank)"""

    def __init__(self, cfg, seed):
        import pamg
        from pamg.solver import local_group
        mesh, S, L = cfg["shape"]
        self.pamg = pamg
        self.mesh = pamg.Mesh.read(path_of(mesh))
        kw = dict(SETS[param_set(seed)], **cfg["kw"])
        if cfg["parts"] == 1:
            self.handles = [pamg.SemiImplicitIterative(self.mesh, S, L, **kw)]
            self.own = [np.arange(self.mesh.U)]
        else:
            owner = self.mesh.x_strip_owner(cfg["parts"])
            self.handles = [pamg.SemiImplicitIterative(self.mesh, S, L, comm=(cfg["parts"], r, None, owner), **kw)
                            for r in range(cfg["parts"])]
            local_group(self.handles)
            self.own = [np.flatnonzero(owner == r) for r in range(cfg["parts"])]
        self.key = (mesh, S, cfg["parts"])
        self._xy = None

    def each(self, fn):
        """fn(handle, rank) on every rank; the list of results"""
        if len(self.handles) == 1:
            return [fn(self.handles[0], 0)]
        from pamg.solver import run_ranks
        out = [None] * len(self.handles)

        def body(h):
            r = self.handles.index(h)
            out[r] = fn(h, r)
        run_ranks(self.handles, body)
        return out

    def gather(self, per_rank):
        """per-rank (.., .., U_r) arrays as one whole-domain array"""
        full = np.empty(per_rank[0].shape[:2] + (self.mesh.U,))
        for own, a in zip(self.own, per_rank):
            full[:, :, own] = a
        return full

    def source(self):
        return self.gather(self.each(lambda h, r: h.get(self.pamg.SOURCE, 1)))

    def xy(self):
        """the level-1 node coordinates of the whole domain (the points pamg_write_vtu writes)"""
        if self._xy is None:
            from test_error_norm import coords
            per = self.each(lambda h, r: coords(h, self.key + (r,)))
            self._xy = self.gather([p[0] for p in per]), self.gather([p[1] for p in per])
        return self._xy

    def states(self):
        def one(h, r):
            st = h.state()
            st["t_overlap"], st["t_overlap_old"] = h.overlap()
            st["tnn_level"] = h.L.pamg_tnn_level(h.h)
            return st
        return self.each(one)

    def close(self):
        for h in self.handles:
            h.close()


def apply_gpu(t, op):
    """the operation on every rank; the per-rank list of what the calls returned"""
    name = op[0]
    if name == "set":
        _, what, level, _ = op
        a = set_array(op, t.handles[0].nsub(level), t.mesh.U)
        return t.each(lambda h, r: h.set(FIELDS[what], level, a[:, :, t.own[r]]))
    if name == "field_norm":
        return t.each(lambda h, r: h.field_norm(FIELDS[op[1]], op[2], op[3]))
    if name == "solve":
        return t.each(lambda h, r: h.solve(-1.0, op[1], op[2], op[3]))
    if name == "smoother":
        return t.each(lambda h, r: h.smoother(op[1], op[2]))
    if name == "run":
        return t.each(lambda h, r: h.run(op[1], op[2]))
    return t.each(lambda h, r: getattr(h, name)(*op[1:]))


def error_bound(x, y, e):
    """field_bound of tests/test_error_norm.py, (3 R + 4) u, is derived for |tnew| <= 1: it counts the rounding of
    the subtraction tnew - sin as one u. A program's tnew is as large as its uploads and cycles make it, and that
    rounding is u times the result on each side (the device's and numpy's): 2 u max|e| is added for it."""
    from test_error_norm import U as EPS, field_bound
    return field_bound(x, y) + 2.0 * EPS * float(e.max())


def check_value(t, o, op, got, model, areas):
    """the value a call returned against the model, with the bounds tests/test_convergence.py and
    tests/test_error_norm.py derive: REF and MAXABS exact, L2 / L1 / L2_MASS within their summation bounds"""
    from test_convergence import assert_l2, expected
    from test_error_norm import U as EPS, assert_l1, assert_mass, mass_sq_exact
    name = op[0]
    S = o.n_split

    def field_kind(v, a, kind, level):
        ref, mx, ss = expected(a)
        if kind == 0:
            assert v == ref, (KIND_NAMES[kind], v, ref)
        elif kind == 1:
            assert v == mx, (KIND_NAMES[kind], v, mx)
        elif kind == 2:
            assert_l2(v, ss, a.size, "L2")
        elif kind == 3:
            assert_l1(v, a, "L1")
        else:
            assert_mass(v, mass_sq_exact(a, areas, S - level + 1), a.shape[1] * a.shape[2], "L2_MASS")

    for v in got:   # every rank receives the global value
        if name == "field_norm":
            _, what, level, kind = op
            field_kind(v, o.get(FIELDS[what], level), kind, level)
        elif name == "residual_norm":
            field_kind(v, model_residual(o, op[1]), op[2], op[1])
        elif name == "get_convergence":
            assert v == max(0.0, float(model.max())), (v, float(model.max()))
        elif name == "solve":
            cycles, value, status, history = v
            assert (cycles, status, len(history)) == (op[1], t.pamg.SOLVE_MAXCYCLES, len(model)), v
            for hv, a in zip(history, model):
                field_kind(hv, a, op[3], 1)
            assert value == history[-1]
        elif name == "error_norm":
            # the device's |tnew - sin(x + y)| is within b = error_bound of numpy's at every node,
            # so its maxima move by at most b, its L1 by n b, its L2 by sqrt(n) b and its mass norm by
            # b sqrt(area) (the norm of the constant b); the reductions add their own summation bounds
            x, y = t.xy()
            e = np.abs(o.get(O.TNEW, 1) - np.sin(x + y))
            b, n, kind = error_bound(x, y, e), e.size, op[1]
            if kind in (0, 1):
                assert abs(v - float(e.max())) <= b, (v, float(e.max()), b)
            elif kind == 2:
                l2 = math.sqrt(math.fsum((e * e).ravel().tolist()))
                assert abs(v - l2) <= math.sqrt(n) * b + n * EPS * l2, (v, l2)
            elif kind == 3:
                l1 = math.fsum(e.ravel().tolist())
                assert abs(v - l1) <= n * b + n * EPS * l1, (v, l1)
            else:
                area = float(sum(areas, Fraction(0)))
                m = math.sqrt(float(mass_sq_exact(e, areas, S)))
                assert abs(v - m) <= b * math.sqrt(area) + (n // 3 + 32) * EPS * m, (v, m)


def run_gpu(cfg, seed, program=None):
    """The program on the handle(s) and the oracle in lock-step. After every operation: every field of every
    level, tnew_nonlin and the level it holds, t_overlap and t_overlap_old are bitwise the oracle's (a rank: the
    oracle's restricted to its un_eles); a refused call raised PamgError and changed nothing."""
    from test_error_norm import areas as exact_areas
    prog = program or generate(cfg, seed)
    t = Target(cfg, seed)
    try:
        o = make_oracle(cfg, seed, t.source())
        areas = exact_areas(o.mesh.X)
        ctx = Ctx(cfg)
        for i, op in enumerate(prog):
            try:
                if op[0] == "illegal":
                    try:
                        apply_gpu(t, op[1])
                    except t.pamg.PamgError as e:
                        assert e.rc < 0
                    else:
                        raise AssertionError("the refused call returned PAMG_OK")
                else:
                    got = apply_gpu(t, op)
                    model = apply_model(o, op)
                    ctx.advance(op)
                    check_value(t, o, op, got, model, areas)
                if op[0] == "get_error":   # the one field the oracle does not hold: against numpy (test_error_norm)
                    x, y = t.xy()
                    err = t.gather(t.each(lambda h, r: h.get(t.pamg.ERROR, 1)))
                    e = np.abs(o.get(O.TNEW, 1) - np.sin(x + y))
                    d = float(np.abs(err - e).max())
                    assert d <= error_bound(x, y, e), ("ERROR", d, error_bound(x, y, e))
                ref = model_state(o)
                for r, st in enumerate(t.states()):
                    assert set(st) == set(ref)
                    for k, v in ref.items():
                        if k == "RHS_L1" and excluded("compare RHS_L1", ctx):
                            continue
                        if k == "tnn_level":
                            assert st[k] == v, (f"rank {r}", k, st[k], v)
                            continue
                        np.testing.assert_array_equal(st[k], v[:, :, t.own[r]], err_msg=f"rank {r} {k}")
            except Failure:
                raise
            except (AssertionError, t.pamg.PamgError) as e:
                _fail(cfg, seed, prog, i, f"{type(e).__name__}: {e}")
    finally:
        t.close()
    return prog
