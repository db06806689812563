"""TEST INFRASTRUCTURE shared by tests/test_tolerance.py (CPU) and tests/test_gpu_tolerance.py (MI355X): the inputs, the
oracle's sequences of relative changes and the rule by which a test chooses its threshold.

A test never hard-codes a tolerance.  It forms the oracle's sequence ``d`` at the check points (float64 numpy, from the
oracle's iterates), takes a target check ``j >= 3`` -- so at least two checks pass without stopping -- and sets
``tol = sqrt(d_{j-1} d_j)``, the geometric mean of the last value that must not stop the loop and the first that must.
The input is acceptable only if every value of the sequence is at least ``max(1 % tol, 4e-5)`` away from ``tol`` and
``d_j`` is the first value below it (`threshold` asserts this; the CPU file runs it for every case of the GPU file, so a
bad input fails there and not on the GPU).  Where the margin comes from: the shipped PD_TV arithmetic is held to 1e-5
relative L2 of the oracle, which moves ``d`` by at most about 2e-5 absolute; 4e-5 is twice that."""
import functools
import os
import sys

import numpy as np

from oracle import tomo_oracle as O

INNER_INTERVAL, INNER_MIN_SAVED = 6, 3
INNER_ITERATIONS = 66
OUTER_ITERATIONS = 15
EPS53 = 2.0 ** -53


def rel_d(v, ref):
    """d = sqrt(sum (v - ref)^2 / sum v^2) in float64 from the float32 values (0 if the numerator is 0, inf if only the
    denominator is)"""
    v64, r64 = np.asarray(v, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    num, den = float(np.sum((v64 - r64) ** 2)), float(np.sum(v64 ** 2))
    if num == 0.0:
        return 0.0
    return float("inf") if den == 0.0 else float(np.sqrt(num / den))


def threshold(seq, j):
    """tol for "stop at the j-th check" (1-based) of the sequence `seq`, by the rule of the module docstring"""
    assert 3 <= j <= len(seq), (j, len(seq))
    tol = float(np.sqrt(seq[j - 2] * seq[j - 1]))
    margin = max(0.01 * tol, 4e-5)
    assert all(abs(v - tol) >= margin for v in seq), ("a value of the sequence is too close to the threshold", tol, seq)
    first = next(i for i, v in enumerate(seq, 1) if v < tol)
    assert first == j, ("the target is not the first value below the threshold", j, first, seq)
    return tol


def never(seq):
    """a threshold below the whole sequence (half its smallest value)"""
    assert min(seq) > 0.0
    return 0.5 * min(seq)


def check_points(iterations=INNER_ITERATIONS):
    return [n for n in range(INNER_INTERVAL, iterations + 1, INNER_INTERVAL) if iterations - n >= INNER_MIN_SAVED]


# ------------------------------------------------------------------------------------------------ inner loops
def phantom(shape, seed=7, sigma=0.05):
    """the central `nz` slices of a 24-slice Shepp-Logan slab [24, n, n] plus Gaussian noise"""
    nz, n, _ = shape
    vol = O.shepp_logan_3d(n, 24)
    vol = (vol + sigma * np.random.default_rng(seed).standard_normal(vol.shape)).astype(np.float32)
    return np.ascontiguousarray(vol[12 - nz // 2:12 - nz // 2 + nz])


# name -> (method, input shape, keyword arguments of the operator, target check j)
INNER_CASES = {
    "pd_3d": ("PD_TV", (24, 40, 40), dict(regularisation_parameter=0.05), 5),
    "pd_3d_half_nonneg_aniso": ("PD_TV", (24, 40, 40), dict(regularisation_parameter=0.05, methodTV=1, nonneg=1,
                                                            half_precision=True), 5),
    "pd_2d": ("PD_TV", (1, 40, 40), dict(regularisation_parameter=0.05), 4),
    "pd_2_slices": ("PD_TV", (2, 40, 40), dict(regularisation_parameter=0.05), 4),
    # z-slabs: 22 slices over 2 ranks (11 + 11) and over 3 (8 + 7 + 7: uneven, with an interior rank)
    "slab_pd_3d": ("PD_TV", (22, 40, 40), dict(regularisation_parameter=0.05), 4),
    "slab_pd_3d_half_nonneg_aniso": ("PD_TV", (22, 40, 40), dict(regularisation_parameter=0.05, methodTV=1, nonneg=1,
                                                                 half_precision=True), 5),
    "slab_rof_3d": ("ROF_TV", (22, 40, 40), dict(regularisation_parameter=0.05, time_marching_parameter=0.005), 5),
    "rof_3d": ("ROF_TV", (24, 40, 40), dict(regularisation_parameter=0.05, time_marching_parameter=0.005), 4),
    "rof_2d_half": ("ROF_TV", (1, 40, 40), dict(regularisation_parameter=0.05, time_marching_parameter=0.005,
                                                half_precision=True), 3),
}


def inner_input(name):
    shape = INNER_CASES[name][1]
    data = phantom(shape)
    return data[0] if shape[0] == 1 else data


def inner_oracle(name, iterations):
    method, _, kw, _ = INNER_CASES[name]
    data = inner_input(name)
    if iterations == 0:
        return data
    return (O.pd_tv if method == "PD_TV" else O.rof_tv)(data, iterations=iterations, **kw)


@functools.lru_cache(maxsize=None)
def inner_sequence(name):
    """the oracle's d at the check points of a 66-iteration call: d_n compares iterate n with iterate n - 6"""
    prev, seq = inner_oracle(name, 0), []
    for n in check_points():
        cur = inner_oracle(name, n)
        seq.append(rel_d(cur, prev))
        prev = cur
    return tuple(seq)


def inner_plan(name):
    """(tol, iterations the oracle's sequence stops after, the d it stops on, a tol that is never met)"""
    seq, j = inner_sequence(name), INNER_CASES[name][3]
    return threshold(seq, j), check_points()[j - 1], seq[j - 1], never(seq)


# ------------------------------------------------------------------------------------------------ outer loops
NZ, N, NA = 6, 32, 48
ANGLES = np.linspace(0, np.pi, NA, endpoint=False)
PD_REG = dict(method="PD_TV", regul_param=0.002, iterations=10, methodTV=0, PD_LipschitzConstant=12.0, exact_roundings=True)
ROF_REG = dict(method="ROF_TV", regul_param=0.002, iterations=8, time_marching_step=0.002)


def _case(driver, os=1, fid="LS", alg=None, reg=None, j=3, nz=NZ):
    return dict(driver=driver, os=os, fid=fid, alg=alg or {}, reg=reg, j=j, nz=nz)


# j: the outer iteration the threshold is chosen to stop after
OUTER_CASES = {
    "fista_os1": _case("FISTA", j=8),
    "fista_os4_pdtv": _case("FISTA", 4, alg=dict(nonnegativity=True), reg=PD_REG, j=3),   # (flattens near 2.4e-3 from iteration 4 on)
    "fista_os4_roftv": _case("FISTA", 4, reg=ROF_REG, j=6),
    "fista_pwls": _case("FISTA", fid="PWLS", j=8),
    "admm_os1_pdtv": _case("ADMM", alg=dict(nonnegativity=True), reg=PD_REG, j=8),
    "admm_os4": _case("ADMM", 4, j=6),
    "osem_os4": _case("OSEM", 4, j=6),
    "sirt": _case("SIRT", j=8),
    "cgls": _case("CGLS", j=6),
    "landweber": _case("Landweber", alg=dict(tau_step_lanweber=2e-4), j=8),
}
GPU_OUTER = sorted(OUTER_CASES)
# both tolerances at once: 30 inner iterations, so the TV operator checks after 6, 12, 18 and 24
BOTH_REG = dict(PD_REG, iterations=30)
OUTER_CASES["both_fista_os4_pdtv"] = _case("FISTA", 4, alg=dict(nonnegativity=True), reg=BOTH_REG, j=3)
# z-slabs: 10 slices over 2 ranks (5 + 5) and over 3 (4 + 3 + 3: uneven, with an interior rank)
OUTER_CASES["slab_fista_os4_pdtv"] = _case("FISTA", 4, alg=dict(nonnegativity=True), reg=BOTH_REG, j=3, nz=10)
OUTER_CASES["slab_admm_os1_roftv"] = _case("ADMM", reg=dict(ROF_REG, iterations=30, regul_param=0.01, time_marching_step=0.005),
                                           j=6, nz=10)
CGLS_TOL = 1e-4   # the bound tests/test_gpu_recon.py holds CGLS to (inner products accumulate in another order)


@functools.lru_cache(maxsize=None)
def sinogram(nz=NZ):
    """noisy, non-negative projections of the phantom, [nz, NA, N]"""
    sino = O.shepp_logan_sino(N, nz, N, ANGLES) / N
    sino = sino + 0.01 * np.random.default_rng(0).standard_normal(sino.shape)
    return np.ascontiguousarray(np.maximum(sino, 0.0), dtype=np.float32)


@functools.lru_cache(maxsize=None)
def projector(os_number, nz=NZ):
    return O.Projector(nz, N, N, ANGLES, 0.0, os_number)


@functools.lru_cache(maxsize=None)
def lipschitz(os_number, nz=NZ):
    x1 = np.random.default_rng(1).standard_normal((nz, N, N)).astype(np.float32)
    return O.power_method(projector(os_number, nz), x1)


def _simple_iterates(driver, alg, iterations, nz):
    """Landweber / SIRT / CGLS as the reference writes them (methodsIR_CuPy.py:128-309), on the oracle's operators: the
    loops tests/test_gpu_recon.py compares with, yielding every iterate"""
    P, sino = projector(1, nz), sinogram(nz)
    shape = (nz, N, N)
    if driver == "Landweber":
        x = np.zeros(shape, np.float32)
        for _ in range(iterations):
            x = x - np.float32(alg["tau_step_lanweber"]) * P.bp(P.fp(x) - sino)
            yield x
    elif driver == "SIRT":
        with np.errstate(divide="ignore"):
            R = np.nan_to_num(np.float32(1) / P.fp(np.ones(shape, np.float32)), nan=1.0, posinf=1.0, neginf=1.0)
            Cm = np.nan_to_num(np.float32(1) / P.bp(np.ones_like(sino)), nan=1.0, posinf=1.0, neginf=1.0)
        x = np.ones(shape, np.float32)
        for _ in range(iterations):
            x = x + Cm * P.bp(R * (sino - P.fp(x)))
            yield x
    else:
        x = np.zeros(nz * N * N, np.float32)
        d = P.bp(sino).ravel()
        normr2 = np.inner(d, d)
        r = sino.ravel().copy()
        for _ in range(iterations):
            Ad = P.fp(d.reshape(shape)).ravel()
            alpha = normr2 / np.inner(Ad, Ad)
            x = x + alpha * d
            r = r - alpha * Ad
            s = P.bp(r.reshape(sino.shape)).ravel()
            normr2_new = np.inner(s, s)
            d = s + (normr2_new / normr2) * d
            normr2 = normr2_new
            yield x.reshape(shape)


def outer_start(name):
    c = OUTER_CASES[name]
    return np.full((c["nz"], N, N), 1.0 if c["driver"] in ("OSEM", "SIRT") else 0.0, np.float32)


def outer_oracle(name, iterations):
    """the oracle's loop of the case run for `iterations` outer iterations"""
    c = OUTER_CASES[name]
    if iterations == 0:
        return outer_start(name)
    P, b = projector(c["os"], c["nz"]), sinogram(c["nz"])
    nonneg = bool(c["alg"].get("nonnegativity", False))
    if c["driver"] == "FISTA":
        return O.fista(P, b, iterations, lipschitz(c["os"], c["nz"]), nonneg, c["reg"], c["fid"])
    if c["driver"] == "ADMM":
        return O.admm(P, b, iterations, lipschitz(c["os"], c["nz"]), 1.0, 1.6, nonneg, c["reg"], c["fid"])
    if c["driver"] == "OSEM":
        return O.osem(P, b, iterations, nonneg, c["reg"])
    *_, last = _simple_iterates(c["driver"], c["alg"], iterations, c["nz"])
    return last


# ---- the oracle's loops with the proximal calls following the inner rule, or running given iteration counts
class _prox_as:
    """for the duration of the block the oracle's loops call `fn(X, reg, nonneg_regul, plain_prox)` as their proximal step"""

    def __init__(self, fn):
        self.fn = fn

    def __enter__(self):
        self.keep = O.prox
        O.prox = lambda X, reg, nonneg_regul: self.fn(X, reg, nonneg_regul, self.keep)

    def __exit__(self, *exc):
        O.prox = self.keep
        return False


def prox_sequence(X, reg, nonneg_regul, plain_prox=None):
    """the oracle's d at the check points of ONE proximal call"""
    plain_prox = plain_prox or O.prox
    prev, seq = X, []
    for n in check_points(reg["iterations"]):
        cur = plain_prox(X, dict(reg, iterations=n), nonneg_regul)
        seq.append(rel_d(cur, prev))
        prev = cur
    return seq


def _prox_with_rule(tol, counts):
    def fn(X, reg, nonneg_regul, plain_prox):
        prev = X
        for n in check_points(reg["iterations"]):
            cur = plain_prox(X, dict(reg, iterations=n), nonneg_regul)
            if rel_d(cur, prev) < tol:
                counts.append(n)
                return cur
            prev = cur
        counts.append(reg["iterations"])
        return plain_prox(X, reg, nonneg_regul)
    return fn


def outer_oracle_inner_rule(name, iterations, inner_tol):
    """(volume, inner iterations of every proximal call) of the oracle's loop with the inner tolerance on"""
    counts = []
    with _prox_as(_prox_with_rule(inner_tol, counts)):
        vol = outer_oracle(name, iterations)
    return vol, counts


def outer_oracle_counts(name, iterations, counts):
    """the oracle's loop with the k-th proximal call running counts[k] iterations"""
    todo = list(counts)
    with _prox_as(lambda X, reg, nonneg_regul, plain: plain(X, dict(reg, iterations=todo.pop(0)), nonneg_regul)):
        vol = outer_oracle(name, iterations)
    assert not todo, "more proximal calls were recorded than the loop makes"
    return vol


class _Captured(Exception):
    pass


@functools.lru_cache(maxsize=None)
def first_prox_sequence(name):
    """the oracle's inner sequence of the FIRST proximal call of the case's loop"""
    def capture(X, reg, nonneg_regul, plain_prox):
        raise _Captured(prox_sequence(X, reg, nonneg_regul, plain_prox))
    try:
        with _prox_as(capture):
            outer_oracle(name, 1)
    except _Captured as e:
        return tuple(e.args[0])
    raise AssertionError("the case makes no proximal call")


def inner_tolerance_of(name, j=3):
    """the inner tolerance of a case with both tolerances on: "stop at the j-th check of the first proximal call" (with 30
    requested iterations and j = 3: at the 18th)"""
    return threshold(first_prox_sequence(name), j)


@functools.lru_cache(maxsize=None)
def outer_iterates(name, inner_tol=None):
    """every iterate v_0 .. v_15 of the oracle's loop (inner_tol: with the inner rule on)"""
    c = OUTER_CASES[name]
    if c["driver"] in ("Landweber", "SIRT", "CGLS"):
        return (outer_start(name),) + tuple(np.array(x, np.float32)
                                           for x in _simple_iterates(c["driver"], c["alg"], OUTER_ITERATIONS, c["nz"]))
    if inner_tol is not None:
        return tuple(outer_oracle_inner_rule(name, k, inner_tol)[0] for k in range(OUTER_ITERATIONS + 1))
    return tuple(outer_oracle(name, k) for k in range(OUTER_ITERATIONS + 1))


def outer_sequence(name, inner_tol=None):
    v = outer_iterates(name, inner_tol)
    return tuple(rel_d(v[k], v[k - 1]) for k in range(1, len(v)))


def outer_plan(name, inner_tol=None):
    """(tol, outer iterations the oracle's sequence stops after, a tol that is never met)"""
    seq, j = outer_sequence(name, inner_tol), OUTER_CASES[name]["j"]
    return threshold(seq, j), j, never(seq)


def outer_dicts(name, tolerance=None, reg_tolerance=None, lipschitz_const=None):
    """(_data_ without the projections, _algorithm_, _regularisation_) of a case"""
    c = OUTER_CASES[name]
    a = dict(c["alg"], iterations=OUTER_ITERATIONS, recon_mask_radius=None)
    if c["driver"] in ("FISTA", "ADMM"):
        a["lipschitz_const"] = lipschitz(c["os"], c["nz"]) if lipschitz_const is None else lipschitz_const
    if tolerance is not None:
        a["tolerance"] = tolerance
    r = None if c["reg"] is None else dict(c["reg"])
    if r is not None and reg_tolerance is not None:
        r["tolerance"] = reg_tolerance
    return {"data_axes_labels_order": ["detY", "angles", "detX"], "data_fidelity": c["fid"]}, a, r


def make_rt(name, device=0, nz=None):
    from tomobar_amd.methodsIR_CuPy import RecToolsIRCuPy
    c = OUTER_CASES[name]
    return RecToolsIRCuPy(N, 0, c["nz"] if nz is None else nz, 0.0, ANGLES, N, device, c["os"] if c["os"] > 1 else None)


def run_driver(rt, name, projections, tolerance=None, reg_tolerance=None, iterations=None):
    """call the case's driver on a RecToolsIRCuPy object; `projections` in the array type of the backend"""
    c = OUTER_CASES[name]
    d, a, r = outer_dicts(name, tolerance, reg_tolerance)
    d["projection_data"] = projections
    if iterations is not None:
        a["iterations"] = iterations
    fn = getattr(rt, c["driver"])
    return fn(d, a, r) if c["driver"] in ("FISTA", "ADMM", "OSEM") else fn(d, a)


def close_lists(got, want, count):
    """two lists of relative changes agree to count * 2^-53 relative (sums of `count` non-negative doubles in any order)"""
    return len(got) == len(want) and all(abs(g - w) <= count * EPS53 * abs(w) for g, w in zip(got, want))


# ------------------------------------------------------------------------------------------------ z-slab ranks
def _start_rank(rank, world, port, backend):
    """one rank of a gloo group; backend "cpu": the oracle stand-ins on host tensors, "gpu": the library, the ranks
    sharing cuda:0 and staging their ghost planes through the host (the pattern of tests/test_gpu_slab_fista.py)"""
    import torch
    import torch.distributed as dist
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    if backend == "gpu":
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    if backend == "cpu":
        import _cpu_backend_tol
        _cpu_backend_tol.install(whole_volume_tv=False)
        return None
    from tomobar_amd import ops
    ops.set_variant("pdtv", 22)   # the reference's roundings: the comparison with the whole-volume oracle is bit for bit
    return torch.device("cuda", 0)


def _host(t):
    return t.detach().cpu().numpy()


def slab_inner_plan(name):
    """computed once by the test process and handed to the ranks (the ranks' CPUs are shared)"""
    tol, stop, d_stop, never_tol = inner_plan(name)
    return dict(tol=tol, stop=stop, d_stop=d_stop, never=never_tol, want_stop=inner_oracle(name, stop),
                want_full=inner_oracle(name, INNER_ITERATIONS))


def slab_inner_worker(rank, world, port, name, backend, plan):
    """pd_tv_slab / rof_tv_slab with a tolerance: every rank stops after the iteration the WHOLE volume's sequence stops
    after, and its planes are those of the unsharded run of that many iterations"""
    import torch
    import torch.distributed as dist
    dev = _start_rank(rank, world, port, backend)
    try:
        from tomobar_amd.slab import SlabComm, pd_tv_slab, rof_tv_slab, slab_bounds
        method, shape, kw, _ = INNER_CASES[name]
        whole = inner_input(name)
        z0, z1 = slab_bounds(shape[0], world, rank)
        mine = torch.from_numpy(whole[z0:z1].copy())
        mine = mine if dev is None else mine.to(dev)
        comm = SlabComm(rank, world, dev)

        def run(tolerance, info):
            if method == "PD_TV":
                return pd_tv_slab(mine, comm, kw["regularisation_parameter"], INNER_ITERATIONS, kw.get("methodTV", 0),
                                  kw.get("nonneg", 0), 8.0, kw.get("half_precision", False), tolerance=tolerance, info=info)
            return rof_tv_slab(mine, comm, kw["regularisation_parameter"], INNER_ITERATIONS, kw["time_marching_parameter"],
                               kw.get("half_precision", False), tolerance=tolerance, info=info)
        info = {}
        got = _host(run(plan["tol"], info))
        assert info["iterations_done"] == plan["stop"], (rank, info, plan["stop"])
        assert abs(info["rel_change"] - plan["d_stop"]) <= whole.size * EPS53 * plan["d_stop"], (rank, info, plan["d_stop"])
        want = plan["want_stop"][z0:z1]
        assert np.array_equal(got, want), (rank, float(np.abs(got - want).max()))
        info = {}
        got = _host(run(plan["never"], info))
        assert info["iterations_done"] == INNER_ITERATIONS, (rank, info)
        assert np.array_equal(got, plan["want_full"][z0:z1]), rank
    finally:
        dist.destroy_process_group()


def slab_outer_plan(name):
    inner_tol = inner_tolerance_of(name)
    tol, stop, _ = outer_plan(name, inner_tol)
    want, counts = outer_oracle_inner_rule(name, stop, inner_tol)
    return dict(inner_tol=inner_tol, tol=tol, stop=stop, want=want, counts=counts,
                seq=list(outer_sequence(name, inner_tol)[:stop]), b=sinogram(OUTER_CASES[name]["nz"]),
                lipschitz=lipschitz(OUTER_CASES[name]["os"], OUTER_CASES[name]["nz"]))


def slab_outer_worker(rank, world, port, name, backend, plan):
    """a driver with rt.slab set and BOTH tolerances on: all ranks stop after the outer iteration the whole volume's
    sequence stops after, every proximal call after the whole volume's count, planes equal to the unsharded run"""
    import torch
    import torch.distributed as dist
    dev = _start_rank(rank, world, port, backend)
    try:
        from tomobar_amd.slab import SlabComm, slab_bounds
        c = OUTER_CASES[name]
        z0, z1 = slab_bounds(c["nz"], world, rank)
        rt = make_rt(name, nz=z1 - z0)
        rt.slab = SlabComm(rank, world, dev)
        b = torch.from_numpy(plan["b"][z0:z1].copy())
        d, a, r = outer_dicts(name, plan["tol"], plan["inner_tol"], lipschitz_const=plan["lipschitz"])
        d["projection_data"] = b if dev is None else b.to(dev)
        got = _host(getattr(rt, c["driver"])(d, a, r))
        run, want = rt.last_run, plan["want"]
        assert run["iterations_done"] == plan["stop"] and run["converged"], (rank, run, plan["stop"])
        assert run["prox_iterations"] == plan["counts"], (rank, run["prox_iterations"], plan["counts"])
        assert close_lists(run["rel_change"], plan["seq"], want.size), (rank, run)
        assert np.array_equal(got, want[z0:z1]), (rank, float(np.abs(got - want[z0:z1]).max()))
    finally:
        dist.destroy_process_group()
