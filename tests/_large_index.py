"""TEST INFRASTRUCTURE: what it takes to hold a kernel to its oracle on an array of more than 2^31 elements -- the shapes,
the memory budget, the periodic-volume check and the dyadic data of the vector kernels.  No GPU on import:
tests/test_large_index.py proves on the CPU every property the MI355X run relies on (tests/test_gpu_large_index.py).

The idea.  An operator whose iteration reaches rho planes along the tiled axis, run for n iterations on an input that
repeats with period p along that axis (`in[z] = base[z % p]`), returns

  * on every plane z of [n rho, len - n rho) a value that depends on input planes within +- n rho only, so out[z] has the
    bits of out[z + p] wherever both lie in that range;
  * on the planes [0, W - n rho) what the oracle returns for the first W = 2 n rho + 2 p input planes (the bottom face and
    one whole interior period), and on the last W - n rho planes what it returns for the last W.

`periodic` checks every interior plane against the period [n rho, n rho + p) on the device and the two windows -- the
first of which holds that period -- against the oracle on the host: the whole output is held to the oracle bit for bit for
the price of 2 W planes of host work.  A plane offset
that wraps by a power of two lands on another plane AND another in-plane position as long as the plane size divides no
threshold (`plane_crossings`), so the periodic volume sees what a z-invariant one cannot.

The tiled axis is z of a volume, y of a 2-D image (a "plane" is then a row), the slice index of a slice-wise operator
(rho = 0) or the one axis of a vector (rho = 0, a plane is one element)."""
import collections

import numpy as np

from _edge_shapes import LAUNCHES, ceil_div   # the launch grid is restated once, there

# elements; for a float array: the signed byte offset, the unsigned byte offset, the signed and the unsigned element index
THRESHOLDS = (2 ** 29, 2 ** 30, 2 ** 31, 2 ** 32)

PLANE = (100, 250)            # (dy, dx) of the tall volumes: 25 000 elements, ragged in x and y for every launch
PAST = 11                     # planes of a tall volume from the one the threshold falls into to the last, inclusive
PERIOD = 7                    # planes (rows) of a period: a small prime


def tall_shape(threshold):
    """(dz, 100, 250) with the element `threshold` strictly inside plane dz - PAST"""
    return (threshold // (PLANE[0] * PLANE[1]) + PAST,) + PLANE


TALL = tall_shape(2 ** 31)                 # (85910, 100, 250): 2 147 750 000 voxels
FLAT = (32774, 16381)                      # 536 870 894 elements, 18 below 2^29: the largest plane a descriptor addresses
FLAT_REFUSED = (32775, 16381)              # 536 887 275 >= 2^29
VECTOR = 2 ** 32 + 4099                    # floats: the element-wise, reduction and stream kernels
# nz a multiple of neither 4 nor 16 (ragged slice quad and z-brick); vol = nz n n, sino = nz na nu
PROJ_PERIOD = 5                                        # vol[z] = base[z % 5]
PROJ_VOLUME = dict(nz=8203, n=512, nu=512, na=16)      # nz n n = 2 150 367 232 > 2^31
PROJ_SINO = dict(nz=8203, n=64, nu=512, na=512)        # nz na nu = 2 150 367 232 > 2^31

# The footprint test_full_size_tv_on_z_invariant_volume[(1100, 1536, 1536)] (tests/test_gpu_fullsize.py) takes: the input
# and the output of 1100 * 1536 * 1536 * 4 = 10 380 902 400 bytes each (a multiple of 256) and tomo_pdtv_scratch_bytes of
# that shape with float32 duals = 2 U arrays + 2 * 3 dual arrays of the same size + 8 * 69 888 bytes of skew:
# 10 * 10 380 902 400 + 559 104.  tests/test_large_index.py recomputes it from the library.
BUDGET = 103_809_583_104


def numel(shape):
    return int(np.prod(np.atleast_1d(shape), dtype=np.int64))


def plane_elems(shape):
    """elements of one index of the tiled (first) axis"""
    shape = tuple(np.atleast_1d(shape))
    return numel(shape[1:]) if len(shape) > 1 else 1


def crossed(shape):
    """the thresholds an array of `shape` has an element at"""
    return tuple(t for t in THRESHOLDS if numel(shape) > t)


def plane_crossings(shape):
    """{threshold: (plane, offset inside it)} for every threshold crossed"""
    pl = plane_elems(shape)
    return {t: divmod(t, pl) for t in crossed(shape)}


# ------------------------------------------------------------------------------------------------ memory
SCRATCH = {  # op -> (C symbol, further arguments after dx, dy, dz, nd)
    "NDF": ("tomo_ndf_scratch_bytes", ()), "Diff4th": ("tomo_diff4th_scratch_bytes", ()),
    "LLT_ROF": ("tomo_llt_rof_scratch_bytes", ()), "TGV": ("tomo_tgv_scratch_bytes", ()),
    "ROF_TV": ("tomo_roftv_scratch_bytes", ()), "PD_TV": ("tomo_pdtv_scratch_bytes", (0,)),
    "PD_TV_half": ("tomo_pdtv_scratch_bytes", (1,)), "NLTV": ("tomo_nltv_scratch_bytes", ()),
    "WAVELETS": ("tomo_wavelet_scratch_bytes", ()),
}


def footprint(op, shape, arrays=2):
    """bytes on the device while `op` runs on float32 arrays of `shape`: `arrays` of them (the input and the output unless
    the operator takes more) and what the library allocates itself -- its tomo_*_scratch_bytes for the names of SCRATCH;
    "PD_TV_slices" / "ROF_TV_slices"; nothing for any other name (the vector kernels and the PDHG / SPDHG steps work on the
    caller's arrays alone)"""
    from tomobar_amd import _lib
    lib = _lib.lib()
    shape = tuple(np.atleast_1d(shape))
    total = arrays * 4 * numel(shape)
    nd = len(shape)
    if op in SCRATCH and nd in (2, 3):
        dz, dy, dx = (1,) * (3 - nd) + shape
        sym, more = SCRATCH[op]
        total += int(getattr(lib, sym)(dx, dy, dz, nd, *more))
    elif op == "PD_TV_slices":
        total += int(lib.tomo_pdtv_slices_scratch_bytes(shape[2], shape[1], shape[0], 0))
    elif op == "ROF_TV_slices":
        total += int(lib.tomo_roftv_slices_scratch_bytes(shape[2], shape[1], shape[0]))
    return total


def largest_tall(op, arrays=2):
    """the tall shape of the largest threshold, 2^31 at most, whose footprint fits BUDGET"""
    for t in (2 ** 31, 2 ** 30, 2 ** 29):
        if footprint(op, tall_shape(t), arrays) <= BUDGET:
            return tall_shape(t)
    raise AssertionError(f"{op} does not fit the budget at 2^29 elements")


# ------------------------------------------------------------------------------------------------ the launch grids
def march_launches(nd):
    """the launches of tests/_edge_shapes.LAUNCHES that take an array of `nd` dimensions"""
    return [L for L in LAUNCHES.values() if nd in L.dims]


def chunk_cap(L, nout):
    """the cap nout / min_planes on the chunk count of a z-march launch"""
    return ceil_div(nout, L.m)


# ------------------------------------------------------------------------------------------------ periodic arrays
def window(base, z0, z1):
    """planes [z0, z1) of the array tiled from `base` ([p, ...]) on the host"""
    return np.ascontiguousarray(base[np.arange(z0, z1) % base.shape[0]])


def _bits(t):
    import torch
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def tiled(base_dev, axis_len, out=None):
    """the device array of `axis_len` planes with plane z = base_dev[z % p], written period by period (no temporary larger
    than `base_dev`'s expansion over one chunk)"""
    import torch
    p = base_dev.shape[0]
    if out is None:
        out = torch.empty((axis_len,) + tuple(base_dev.shape[1:]), dtype=base_dev.dtype, device=base_dev.device)
    full = axis_len // p
    if full:
        out[:full * p].view((full, p) + tuple(base_dev.shape[1:])).copy_(base_dev.unsqueeze(0))
    if axis_len % p:
        out[full * p:].copy_(base_dev[:axis_len % p])
    return out


def _where(z, plane):
    off = z * plane
    if plane == 1:
        return f"element {z} (= " + ", ".join(f"{z % t} mod 2^{t.bit_length() - 1}" for t in THRESHOLDS) + ")"
    return f"plane {z} (its first element is element {off} = " + ", ".join(
        f"{off % t} mod 2^{t.bit_length() - 1}" for t in THRESHOLDS) + ")"


def first_unequal_plane(x, ref, z0, z1, phase, chunk_elems=1 << 27):
    """None if plane z of `x` has the bits of ref[(z - phase) % p] for every z of [z0, z1), else the first z that has not.
    Compared on the device of `x` in chunks of about `chunk_elems` elements; (z0 - phase) % p must be 0."""
    p = ref.shape[0]
    assert (z0 - phase) % p == 0
    plane = plane_elems(x.shape)
    rb = _bits(ref).reshape(1, p, plane)
    per_chunk = max(1, chunk_elems // (p * plane)) * p
    for a in range(z0, z1, per_chunk):
        b = min(a + per_chunk, z1)
        full = (b - a) // p
        xb = _bits(x[a:b]).reshape(b - a, plane)
        bad = None
        if full:
            ne = (xb[:full * p].view(full, p, plane) != rb).any(dim=2)
            if bool(ne.any()):
                bad = int(ne.reshape(-1).nonzero()[0])
        if bad is None and (b - a) % p:
            ne = (xb[full * p:] != rb[0, :(b - a) % p]).any(dim=1)
            if bool(ne.any()):
                bad = full * p + int(ne.nonzero()[0])
        if bad is not None:
            return a + bad
    return None


def same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    u = {4: np.uint32, 2: np.uint16, 1: np.uint8}[got.dtype.itemsize]
    g, w = np.ascontiguousarray(got).view(u), np.ascontiguousarray(want).view(u)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        raise AssertionError((what, f"{len(bad)} of {got.size} values differ, first at {tuple(bad[0])}"))


def _window(compare, got, want, z0, plane, what):
    """compare(got, want, what); a failure also names the first plane (from z0) whose bits differ"""
    try:
        compare(got, want, what)
    except AssertionError as e:
        n = got.shape[0]
        g, w = (np.ascontiguousarray(a).reshape(n, -1).view(np.uint32) for a in (got, want))
        ne = np.flatnonzero((g != w).any(axis=1))
        at = _where(z0 + int(ne[0]), plane) if ne.size else "no plane bit for bit"
        raise AssertionError((what, "differs from the oracle at " + at, e.args)) from e


def _as_list(v):
    return list(v) if isinstance(v, (list, tuple)) else [v]


def periodic(op_call, oracle_call, base, axis_len, reach, *, outputs=1, compare=same_bits, device="cuda", what="", scratch=()):
    """Hold an operator to its oracle on arrays of `axis_len` planes tiled from `base`; asserts, returns nothing.

    base         the period on the host, [p, ...], or a tuple of such arrays (one per input of the operator, the same p)
    op_call      op_call(ins, outs): runs the operator on the device.  `ins`: the tiled inputs; `outs`: `outputs` NaN-filled
                 float32 arrays like the first input.  It returns None (the results are `outs`) or the list of the tensors
                 that hold the results -- an operator that works in place returns the inputs it updated, which are then
                 exempt from the check that every input still holds its bits.
    oracle_call  oracle_call(*windows) -> the result(s) on the host for the same planes of every input
    reach        n rho: the planes an output plane depends on either side (0: plane by plane)
    scratch      indices of the inputs the operator may overwrite with something nobody reads
    compare      compare(got, want, what) of a window on the host (bit equality unless the operator ships relaxed
                 arithmetic); the periodicity of the interior is bit for bit always

    A failure names the first plane that differs and the element offset of its first value modulo each threshold."""
    import torch
    bases = [np.ascontiguousarray(b) for b in _as_list(base)]
    p = bases[0].shape[0]
    assert all(b.shape[0] == p for b in bases)
    W = 2 * reach + 2 * p
    assert axis_len >= W + p, (axis_len, W)
    bases_dev = [torch.from_numpy(b).to(device) for b in bases]
    ins = [tiled(b, axis_len) for b in bases_dev]
    outs = [torch.full_like(ins[0], float("nan")) for _ in range(outputs)]
    res = op_call(ins, outs)
    res = outs if res is None else _as_list(res)
    if device != "cpu":
        torch.cuda.synchronize()
    for k, (x, b) in enumerate(zip(ins, bases_dev)):      # 1. the inputs the operator only reads hold their bits
        if k in scratch or any(x is r for r in res):
            continue
        z = first_unequal_plane(x, b, 0, axis_len, 0)
        assert z is None, (what, f"input {k} was written at " + _where(z, plane_elems(x.shape)))
    # 2. every interior plane has the bits of the period [reach, reach + p) (first, so that a failure names the FIRST plane
    # that went wrong, not one of the last window)
    lo = [window(b, 0, W) for b in bases]
    want_lo = _as_list(oracle_call(*lo))
    assert len(want_lo) == len(res), (what, len(want_lo), len(res))

    def first_window(k):
        _window(compare, res[k][:W - reach].cpu().numpy(), np.ascontiguousarray(want_lo[k][:W - reach]), 0, plane_elems(res[k].shape),
                (what, k, "the first planes"))

    for k, r in enumerate(res):
        assert r.shape[0] == axis_len
        ref = r[reach:reach + p].clone()
        z = first_unequal_plane(r, ref, reach, axis_len - reach, reach)
        if z is not None:
            first_window(k)   # (if the period compared with is itself wrong, say that instead)
        assert z is None, (what, f"output {k} is not periodic at " + _where(z, plane_elems(r.shape)) +
                           f": it differs from plane {reach + (z - reach) % p}")
    # 3. the two windows against the oracle: the bottom face with that period, and the top face
    hi = [window(b, axis_len - W, axis_len) for b in bases]
    want_hi = _as_list(oracle_call(*hi))
    for k, r in enumerate(res):
        plane = plane_elems(r.shape)
        first_window(k)
        _window(compare, r[axis_len - W + reach:].cpu().numpy(), np.ascontiguousarray(want_hi[k][reach:]), axis_len - W + reach, plane,
                (what, k, "the last planes"))


# ------------------------------------------------------------------------------------------------ dyadic vectors
DYADIC_PERIOD = 8191     # a prime: no power-of-two wrap maps a period onto itself


def dyadic(seed, p=DYADIC_PERIOD, positive=False):
    """`p` float32 values k / 8, integer k in [-16, 16] (in [1, 16] with `positive`), k != 0: every product, sum and square
    of two of them is exact in float32, and a sum of 2^32 + 4099 such terms (each a multiple of 1/64 of magnitude <= 4, so
    at most about 1.1e12 units of 1/64, below 2^53) is exact in float64 in any order"""
    rng = np.random.default_rng(seed)
    k = rng.integers(1, 17, size=p)
    if not positive:
        k = k * rng.choice((-1, 1), size=p)
    return (k / 8.0).astype(np.float32)


def tiled_sum(period_values, n):
    """sum over i < n of period_values[i % p], in float64 (exact for dyadic data): whole periods, then the rest"""
    v = np.asarray(period_values, np.float64)
    full, rest = divmod(n, v.shape[0])
    return float(full * v.sum() + v[:rest].sum())



# ------------------------------------------------------------------------------------------------ the operators
# One record per test id, read by the CPU proof (the oracle in both roles) and by the MI355X run (`gpu` against `oracle`).
#   bases(shape) -> the period of every input on the host, `shape` = (p, ...) of one period
#   oracle(*windows) -> the list of results on the host
#   gpu(ins, outs) -> what periodic's op_call returns;  outputs: NaN-filled arrays it asks for
#   reach: planes either side an output plane depends on;  foot: (name for `footprint`, arrays held while it runs)
#   pd: the first result goes through the `pd_arith` fixture (PD_TV float32 duals ship relaxed arithmetic); half: binary16
Op = collections.namedtuple("Op", "id bases oracle gpu outputs reach foot pd half")


def _field(shape):
    from _tgv_oracle import phantom
    return phantom(shape)


def _noise(shape, seed, amp):
    return (np.random.default_rng(seed).uniform(-amp, amp, shape)).astype(np.float32)


def _nd_view(t, nd):
    """a 2-D image as the [1, ny, nx] volume the PDHG and SPDHG entries take"""
    return t if nd == 3 else t.unsqueeze(0) if hasattr(t, "unsqueeze") else t[None]


def _unview(a, nd):
    return a if nd == 3 else a[0]


def march_ops(nd, iteration_counts=(1, 2)):
    """NDF (one set per penalty, and a fourth), Diff4th, LLT_ROF and TGV"""
    import _diff4th_oracle
    import _llt_rof_oracle
    import _ndf_oracle
    import _tgv_oracle
    out = []
    sets = [("NDF", _ndf_oracle.ORACLE, "ABCD"), ("Diff4th", _diff4th_oracle.ORACLE, "ABC"), ("LLT_ROF", _llt_rof_oracle.ORACLE, "ABC")]
    for name, D, pnames in sets:
        for pname in pnames:
            for n in iteration_counts:
                p = D.PARAMS[pname]

                def gpu(ins, outs, name=name, D=D, p=p, n=n):
                    from tomobar_amd import ops
                    getattr(ops, name.lower())(ins[0], outs[0], *(np.float32(p[k]) for k in D.keys), *(p[k] for k in D.extra), n, 0.0)

                out.append(Op(f"{name}-{pname}-it{n}", lambda s: (_field(s),), lambda w, D=D, p=p, n=n: [D.run(w, iterations=n, **p)],
                              gpu, 1, n * D.GHOST, (name, 2), False, False))
    for pname, P in (("A", _tgv_oracle.PARAMS_A), ("B", _tgv_oracle.PARAMS_B)):
        for n in iteration_counts:
            def gpu(ins, outs, P=P, n=n):
                from tomobar_amd import ops
                ops.tgv(ins[0], outs[0], *_tgv_oracle.scalars(**P), n)

            out.append(Op(f"TGV-{pname}-it{n}", lambda s: (_field(s),), lambda w, P=P, n=n: [_tgv_oracle.tgv(w, iterations=n, **P)],
                          gpu, 1, 2 * n, ("TGV", 2), False, False))
    return out


TV_LAM, ROF_TAU, PD_L = 0.04, 0.005, 12.0   # the parameters of tests/test_gpu_fullsize.py


def _tv_field(shape):
    from _edge_shapes import step_noise
    return step_noise(shape)


def tv_ops(nd):
    """ROF_TV with both dual types; PD_TV at 7 (= 3 + 2 + 2) iterations with both dual types, methodTV 0 / 1, with and without
    the clip, and at 1 iteration (3-D: the single-iteration march) with both dual types, plain and with both switches"""
    from oracle import tomo_oracle as O
    out = []
    for half in (False, True):
        def gpu(ins, outs, half=half):
            from tomobar_amd.regularisersCuPy import ROF_TV_cupy
            ROF_TV_cupy(ins[0], TV_LAM, 3, ROF_TAU, 0, half, out=outs[0])

        out.append(Op(f"ROF_TV-{'f16' if half else 'f32'}-it3", lambda s: (_tv_field(s),),
                      lambda w, half=half: [O.rof_tv(w, TV_LAM, 3, ROF_TAU, half).reshape(w.shape)], gpu, 1, 6, ("ROF_TV", 2), False, half))
    combos = [(7, m, c) for m in (0, 1) for c in (0, 1)] + [(1, 0, 0), (1, 1, 1)]
    if nd == 2:   # pd_rows2d at K = 3, 2, 1: 3, 2 (4 = 2 + 2 takes K = 2 twice) and 1
        combos = [(3, 0, 0), (3, 1, 1), (4, 0, 1), (4, 1, 0), (1, 0, 0), (1, 1, 1)]
    for n, methodTV, nonneg in combos:
        for half in (False, True):
            def gpu(ins, outs, n=n, methodTV=methodTV, nonneg=nonneg, half=half):
                from tomobar_amd.regularisersCuPy import PD_TV_cupy
                PD_TV_cupy(ins[0], TV_LAM, n, methodTV, nonneg, PD_L, 0, half, out=outs[0])

            out.append(Op(f"PD_TV-{'f16' if half else 'f32'}-it{n}-m{methodTV}-c{nonneg}",
                          lambda s, nonneg=nonneg: (_tv_field(s) - (np.float32(0.5) if nonneg else np.float32(0)),),
                          lambda w, n=n, methodTV=methodTV, nonneg=nonneg, half=half:
                          [O.pd_tv(w, TV_LAM, n, methodTV, nonneg, PD_L, half).reshape(w.shape)],
                          gpu, 1, n, ("PD_TV_half" if half else "PD_TV", 2), True, half))
    return out


PDHG_SIGMA, PDHG_TAU, PDHG_LAM, SPDHG_W = 0.25, 0.125, 0.5, 2.0   # dyadic scalars; lam is reached by the duals below


def pdhg_ops(nd):
    """the five TV entries of PDHG and SPDHG, every one with only the arrays it touches.  Inputs: a field, dual fields of
    magnitude up to lam (so that the projection is active on a part of the voxels), steps per voxel in [1/16, 1/4]"""
    import _pdhg_diag_oracle
    import _pdhg_oracle
    import _spdhg_oracle
    def fields(s, n_plain, n_dual, tau=False):
        arrays = [_field(s) if k == 0 else _field(s)[..., ::-1].copy() * np.float32(0.5) for k in range(n_plain)]
        if tau:
            arrays.append((_noise(s, 40, 0.09375) + np.float32(0.15625)).astype(np.float32))
        return tuple(arrays + [_noise(s, 50 + k, 2 * PDHG_LAM) for k in range(n_dual)])

    def V(ts):
        return [_nd_view(t, nd) for t in ts]

    out = []
    for m in (0, 1):
        def gpu(ins, outs, m=m):
            from tomobar_amd import ops
            ops.pdhg_tv_dual(_nd_view(ins[0], nd), V(ins[1:]), PDHG_SIGMA, PDHG_LAM, m)
            return ins[1:]

        out.append(Op(f"pdhg_tv_dual-m{m}", lambda s: fields(s, 1, nd),
                      lambda xb, *q, m=m: [_unview(a, nd) for a in _pdhg_oracle.tv_dual(_nd_view(xb, nd), V(q), PDHG_SIGMA, PDHG_LAM, m)],
                      gpu, 0, 1, ("pdhg", 1 + nd), False, False))

        def gpu(ins, outs, m=m):
            from tomobar_amd import ops
            ops.spdhg_tv_dual(_nd_view(ins[0], nd), V(ins[1:]), V(outs), PDHG_SIGMA, PDHG_LAM, m)
            return list(ins[1:]) + list(outs)

        def orc(x, *q, m=m):
            p, e = _spdhg_oracle.tv_dual_step(_nd_view(x, nd), V(q), PDHG_SIGMA, PDHG_LAM, m)
            return [_unview(a, nd) for a in list(p) + list(e)]

        out.append(Op(f"spdhg_tv_dual-m{m}", lambda s: fields(s, 1, nd), orc, gpu, nd, 1, ("spdhg", 1 + 2 * nd), False, False))
    for c in (0, 1):
        def gpu(ins, outs, c=c):   # x and x-bar are written: x-bar is never read, so it is the NaN-filled array
            from tomobar_amd import ops
            ops.pdhg_primal(_nd_view(ins[0], nd), _nd_view(outs[0], nd), _nd_view(ins[1], nd), V(ins[2:]), PDHG_TAU, c)
            return [ins[0], outs[0]]

        out.append(Op(f"pdhg_primal-c{c}", lambda s: fields(s, 2, nd),
                      lambda x, g, *q, c=c: [_unview(a, nd) for a in _pdhg_oracle.primal(_nd_view(x, nd), _nd_view(g, nd), V(q), PDHG_TAU, c)],
                      gpu, 1, 1, ("pdhg", 3 + nd), False, False))

        def gpu(ins, outs, c=c):
            from tomobar_amd import ops
            ops.pdhg_primal_diag(_nd_view(ins[0], nd), _nd_view(outs[0], nd), _nd_view(ins[1], nd), V(ins[3:]), _nd_view(ins[2], nd), c)
            return [ins[0], outs[0]]

        out.append(Op(f"pdhg_primal_diag-c{c}", lambda s: fields(s, 2, nd, tau=True),
                      lambda x, g, tau, *q, c=c: [_unview(a, nd) for a in
                                                  _pdhg_diag_oracle.primal(_nd_view(x, nd), _nd_view(g, nd), V(q), _nd_view(tau, nd), c)],
                      gpu, 1, 1, ("pdhg", 4 + nd), False, False))

        def gpu(ins, outs, c=c):
            from tomobar_amd import ops
            ops.spdhg_tv_primal(_nd_view(ins[0], nd), _nd_view(ins[1], nd), V(ins[2:]), PDHG_TAU, SPDHG_W, c)
            return [ins[0], ins[1]]

        out.append(Op(f"spdhg_tv_primal-c{c}", lambda s: fields(s, 2, nd),
                      lambda x, z, *e, c=c: [_unview(a, nd) for a in
                                             _spdhg_oracle.tv_primal_step(_nd_view(x, nd), _nd_view(z, nd), V(e), PDHG_TAU, SPDHG_W, c)],
                      gpu, 0, 1, ("spdhg", 2 + nd), False, False))
    return out


NLTV_STACK = tall_shape(2 ** 28)           # (10748, 100, 250): K * nvox passes 2^31 with K = 8 neighbours


def other_footprints():
    """(name for `footprint`, shape, float32 arrays of that shape held) of what runs beside the volume operators: the
    slice-wise operators on TALL taken as 85910 slices (wavelet_forward / inverse hold the pyramid twice: the caller's and
    the oracle period's share is small); the vector kernels, at most five arrays of VECTOR + 1 floats; NLTV, whose tables
    are 8 neighbours * (2 + 2 + 4) bytes = 16 floats per voxel"""
    return [("PD_TV_slices", TALL, 2), ("ROF_TV_slices", TALL, 2), ("WAVELETS", TALL, 2), ("wavelet pyramid", TALL, 5),
            ("vector", (VECTOR + 1,), 5), ("NLTV", NLTV_STACK, 2 + 16)]


def volume_ops(nd):
    return march_ops(nd) + tv_ops(nd) + pdhg_ops(nd)


def op_shape(op, nd):
    """the shape `op` runs at on the MI355X: FLAT in 2-D; in 3-D the tall shape of the largest threshold that fits BUDGET"""
    return FLAT if nd == 2 else largest_tall(*op.foot)
