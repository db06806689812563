"""What the MI355X run past 2^31 elements (tests/test_gpu_large_index.py) relies on, proven without a GPU: the periodic-volume
argument with the reach every operator is given there, the properties of the shapes, the exactness of the dyadic data, the
helper's own failure report, and the refusals that protect the 32-bit buffer descriptors (tests/_large_index.py)."""
import ctypes as C

import numpy as np
import pytest

import _large_index as LI
from _edge_shapes import LAUNCHES

torch = pytest.importorskip("torch")

SMALL = {3: (9, 11), 2: (11,)}      # one period's plane (row) at the small shape; 60 planes (rows) of them
AXIS = 60


def _cpu_call(op):
    """the oracle in the role of the operator: the whole tiled array at once"""
    def call(ins, outs):
        return [torch.from_numpy(np.ascontiguousarray(a)) for a in op.oracle(*(t.numpy() for t in ins))]
    return call


# ------------------------------------------------------------------------------------------------ periodicity and windows
@pytest.mark.parametrize("nd", [3, 2])
def test_the_table_names_every_operator_once(nd):
    ids = [op.id for op in LI.volume_ops(nd)]
    assert len(ids) == len(set(ids))


@pytest.mark.parametrize("nd,op", [(nd, op) for nd in (3, 2) for op in LI.volume_ops(nd)], ids=lambda v: v if isinstance(v, int) else v.id)
def test_interior_is_periodic_and_windows_equal_the_whole_array(nd, op):
    """with the reach the MI355X test uses: in z for the volumes, in y for the 2-D forms"""
    bases = op.bases((LI.PERIOD,) + SMALL[nd])
    LI.periodic(_cpu_call(op), op.oracle, bases, AXIS, op.reach, outputs=op.outputs, device="cpu", what=op.id)


@pytest.mark.parametrize("opid", ["NDF-A-it2", "NDF-B-it2", "NDF-C-it2", "Diff4th-A-it2", "Diff4th-B-it2", "Diff4th-C-it2"])
def test_the_plane_just_outside_the_cone_is_not_periodic(opid):
    """the reach is tight: nobody mends a failure by widening it"""
    op = next(o for o in LI.volume_ops(3) if o.id == opid)
    f = LI.window(op.bases((LI.PERIOD,) + SMALL[3])[0], 0, AXIS)
    out = op.oracle(f)[0]
    z = op.reach - 1
    assert not np.array_equal(out[z].view(np.uint32), out[z + LI.PERIOD].view(np.uint32))
    z = AXIS - op.reach
    assert not np.array_equal(out[z].view(np.uint32), out[z - LI.PERIOD].view(np.uint32))
    with pytest.raises(AssertionError):
        LI.periodic(_cpu_call(op), op.oracle, op.bases((LI.PERIOD,) + SMALL[3]), AXIS, op.reach - 1, device="cpu")


def test_slice_wise_operators_act_slice_by_slice():
    """reach 0 over the slices: the slice-wise TV and the wavelets (the projectors and NLTV are compared slice by slice with the
    oracle's result for the period itself: nothing to prove)"""
    import _slicewise_cases as S
    import _wavelet_oracle as W
    base = LI._field((5, 12, 14))
    cases = [lambda v: S.oracle_slices("PD_TV", v, **S.pd_kwargs(7)), lambda v: S.oracle_slices("ROF_TV", v, **S.rof_kwargs(3)),
             lambda v: W.shrink(v, np.float32(0.5)), lambda v: W.pack(W.forward(v, np.float32(0.5))).reshape(v.shape[0], -1)]
    for fn in cases:
        LI.periodic(lambda ins, outs, fn=fn: [torch.from_numpy(np.ascontiguousarray(fn(ins[0].numpy())))], lambda w, fn=fn: [fn(w)],
                    base, 23, 0, outputs=0, device="cpu")


# ------------------------------------------------------------------------------------------------ the helper reports
def test_periodic_names_the_plane_and_its_offsets():
    op = next(o for o in LI.volume_ops(3) if o.id == "NDF-A-it1")
    bases = op.bases((LI.PERIOD,) + SMALL[3])

    def wrong_plane(ins, outs):   # plane 41 holds plane 40's result: what a wrapped plane offset does
        res = _cpu_call(op)(ins, outs)
        res[0][41] = res[0][40]
        return res

    with pytest.raises(AssertionError) as e:
        LI.periodic(wrong_plane, op.oracle, bases, AXIS, op.reach, device="cpu", what="NDF")
    msg = str(e.value)
    assert "not periodic at plane 41 " in msg and f"element {41 * 99}" in msg and f"{41 * 99 % 2 ** 29} mod 2^29" in msg

    def writes_input(ins, outs):
        ins[0][33, 2, 3] = 0.0
        return _cpu_call(op)(ins, outs)

    with pytest.raises(AssertionError, match="input 0 was written at plane 33 "):
        LI.periodic(writes_input, op.oracle, bases, AXIS, op.reach, device="cpu")

    def leaves_a_plane(ins, outs):   # the NaN prefill shows a plane never written
        outs[0].copy_(_cpu_call(op)(ins, outs)[0])
        outs[0][30] = float("nan")

    with pytest.raises(AssertionError, match="not periodic at plane 30 "):
        LI.periodic(leaves_a_plane, op.oracle, bases, AXIS, op.reach, device="cpu")


def test_a_z_invariant_volume_cannot_see_a_wrong_plane_but_a_periodic_one_does():
    """the gap this suite closes, on the data path: planes fetched through an offset that wraps onto another plane at the
    same in-plane position (a power-of-two plane, as 1024^2 is)"""
    plane_shape, wrap = (8, 16), 2 ** 12     # 128 elements a plane: plane z is fetched from plane z mod 32

    def wrapped(f):   # the plane offset z * plane taken modulo `wrap`: the 32-bit wrap, scaled to the small shape
        flat = f.ravel()
        return np.stack([flat[(z * 128) % wrap:(z * 128) % wrap + 128].reshape(plane_shape) for z in range(f.shape[0])])

    op = next(o for o in LI.volume_ops(3) if o.id == "NDF-A-it1")
    base = op.bases((LI.PERIOD,) + plane_shape)[0]
    # the check of test_full_size_tv_on_z_invariant_volume: every plane equals the first, which equals the 2-D result
    flat = np.ascontiguousarray(np.broadcast_to(base[:1], (AXIS,) + plane_shape))
    got = op.oracle(wrapped(flat))[0]
    assert np.array_equal(got, np.broadcast_to(got[:1], got.shape)) and np.array_equal(got, op.oracle(flat)[0])
    # the periodic volume: plane 32 is fetched from plane 0, so the output differs from plane 31 on (NDF reaches one plane)
    with pytest.raises(AssertionError, match="not periodic at plane 31 "):
        LI.periodic(lambda ins, outs: [torch.from_numpy(op.oracle(wrapped(ins[0].numpy()))[0])], op.oracle, base, AXIS, op.reach, device="cpu")


# ------------------------------------------------------------------------------------------------ the shapes
def test_budget_is_the_footprint_of_the_largest_existing_test():
    assert LI.BUDGET == LI.footprint("PD_TV", (1100, 1536, 1536)) == 10 * 1100 * 1536 * 1536 * 4 + 8 * 69888


SHAPES = {"tall": LI.TALL, "tall 2^30": LI.tall_shape(2 ** 30), "tall 2^29": LI.tall_shape(2 ** 29), "flat": LI.FLAT,
          "vector": (LI.VECTOR,), "projector volume": (LI.PROJ_VOLUME["nz"], LI.PROJ_VOLUME["n"], LI.PROJ_VOLUME["n"]),
          "projector sinogram": (LI.PROJ_SINO["nz"], LI.PROJ_SINO["na"], LI.PROJ_SINO["nu"]),
          "NLTV tables": (8, LI.NLTV_STACK[0], LI.NLTV_STACK[1], LI.NLTV_STACK[2])}
CLAIMS = {"tall": 3, "tall 2^30": 2, "tall 2^29": 1, "flat": 0, "vector": 4, "projector volume": 3, "projector sinogram": 3,
          "NLTV tables": 3}


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_threshold_a_shape_claims_falls_strictly_inside_a_plane(name):
    shape = SHAPES[name]
    assert len(LI.crossed(shape)) == CLAIMS[name], LI.crossed(shape)
    if name == "vector":
        return
    plane = LI.numel(shape[1:]) if name != "NLTV tables" else LI.numel(shape[2:])
    for t in LI.THRESHOLDS:
        if name.startswith("projector"):
            # slices of 2^k elements: a wrap lands on the same position of another slice, which the period of 5 slices sees
            # as long as the distance in slices is no multiple of 5
            assert t % plane == 0 and (t // plane) % LI.PROJ_PERIOD != 0, (name, t, plane)
            continue
        assert t % plane != 0, (name, t, plane)       # the plane size divides no threshold
    if name.startswith("projector"):
        return
    for t, (z, off) in LI.plane_crossings(shape).items():
        assert 0 < off < LI.plane_elems(shape) and z < shape[0], (name, t, z, off)


def test_the_tall_shape_is_the_one_the_issue_states():
    assert LI.TALL == (85910, 100, 250) and LI.numel(LI.TALL) == 2_147_750_000
    assert {t: z for t, (z, _) in LI.plane_crossings(LI.TALL).items()} == {2 ** 29: 21474, 2 ** 30: 42949, 2 ** 31: 85899}
    assert LI.numel(LI.FLAT) == 2 ** 29 - 18 and LI.numel(LI.FLAT_REFUSED) >= 2 ** 29
    for g in (LI.PROJ_VOLUME, LI.PROJ_SINO):
        assert g["nz"] % 4 and g["nz"] % 16


@pytest.mark.parametrize("nd", [3, 2])
def test_every_operator_fits_the_budget_at_its_shape(nd):
    for op in LI.volume_ops(nd):
        shape = LI.op_shape(op, nd)
        assert LI.footprint(op.foot[0], shape, op.foot[1]) <= LI.BUDGET, op.id
        if nd == 3:
            assert (LI.crossed(shape) == LI.THRESHOLDS[:3]) == (not op.id.startswith("TGV")), op.id
    assert LI.largest_tall("TGV") == LI.tall_shape(2 ** 30)          # 16 work arrays: 2^31 does not fit
    for name, shape, arrays in LI.other_footprints():
        assert LI.footprint(name, shape, arrays) <= LI.BUDGET, name


@pytest.mark.parametrize("launch", [L.name for L in LI.march_launches(3)])
def test_the_tall_grid_takes_the_want_driven_chunk_count(launch):
    """the branch of zmarch_grid no other test reaches: `chunks` comes from the waves wanted, not from nout / min_planes"""
    L = LAUNCHES[launch]
    for shape in (LI.TALL, LI.tall_shape(2 ** 30)):
        g = L.grid(shape)
        assert g.tiles_per_xcd >= 2 and (g.gx * g.gy) % 8 != 0, g
        assert 1 < g.chunks < LI.chunk_cap(L, shape[0]), (g, LI.chunk_cap(L, shape[0]))


@pytest.mark.parametrize("launch", [L.name for L in LI.march_launches(2)])
def test_the_flat_grid_has_tens_of_thousands_of_tiles_per_xcd(launch):
    L = LAUNCHES[launch]
    g = L.grid(LI.FLAT)
    if L.rows2d:   # one tile per wave, four waves per block, no XCD numbering: a quarter of a million blocks
        assert g.gx * g.gy > 2 ** 20 and g.blocks > 2 ** 18 and (g.gx * g.gy) % 4 != 0, g
    else:
        assert 10_000 <= g.tiles_per_xcd < 100_000 and (g.gx * g.gy) % 8 != 0, g


# ------------------------------------------------------------------------------------------------ dyadic data
def test_dyadic_sums_do_not_depend_on_the_order_and_float32_arithmetic_is_exact():
    x, y = LI.dyadic(1), LI.dyadic(2)
    assert x.dtype == np.float32 and np.all(x != 0) and np.all(np.abs(x) <= 2) and np.all(x * 8 == np.round(x * 8))
    n = 3 * LI.DYADIC_PERIOD + 17
    v = LI.window(x, 0, n).astype(np.float64)
    w = LI.window(y, 0, n).astype(np.float64)
    for term in (v * v, v * w, (v - w) ** 2):
        fwd, bwd = float(np.sum(term)), float(np.sum(term[::-1]))
        pair = float(np.sum(term[0::2]) + np.sum(term[1::2]))
        assert fwd == bwd == pair
    assert LI.tiled_sum(x.astype(np.float64) ** 2, n) == float(np.sum(v * v))
    a, b = np.float32(0.75), np.float32(-1.5)
    assert np.array_equal((a * x + b * y).astype(np.float64), 0.75 * x.astype(np.float64) - 1.5 * y.astype(np.float64))
    assert np.array_equal((x * y).astype(np.float64), x.astype(np.float64) * y.astype(np.float64))
    # the largest sum of the MI355X run, in units of 1/64, stays below 2^53; every element contributes at least one unit
    assert LI.VECTOR * 4 * 64 < 2 ** 53 and np.all(np.abs(x * y) * 64 >= 1) and np.all((x - y) ** 2 * 64 == np.round((x - y) ** 2 * 64))


# ------------------------------------------------------------------------------------------------ the refusals
P = [C.c_void_p(0x1000 * k) for k in range(1, 9)]   # never dereferenced: every call fails validation
NUL = C.c_void_p(0)
PLANE_LIMIT = "exceeds the 2 GiB a buffer descriptor of the TV kernels addresses"


def _entries():
    """name -> call(dx, dy, null): the entry on a plane of dx x dy, valid in every other argument; with `null` its first
    data pointer is NULL"""
    from tomobar_amd import _lib
    lib = _lib.lib()
    i0, d0 = C.c_int(0), C.c_double(0.0)
    tol = (0.0, C.byref(i0), C.byref(d0), None)     # the tolerance, where it reports, the stream
    pd = (0.25, 0.25, 0.1, 1.0, 3, 0, 0, 0)         # sigma, tau, lt, theta, iterations, methodTV, nonneg, half

    def a(null):
        return NUL if null else P[0]

    e = {}
    e["tomo_pdtv"] = lambda dx, dy, n: lib.tomo_pdtv(0, a(n), P[1], dx, dy, 3, 3, *pd, None)
    e["tomo_pdtv_tol"] = lambda dx, dy, n: lib.tomo_pdtv_tol(0, a(n), P[1], dx, dy, 3, 3, *pd, *tol)
    e["tomo_roftv"] = lambda dx, dy, n: lib.tomo_roftv(0, a(n), P[1], dx, dy, 3, 3, 0.04, 0.005, 3, 0, None)
    e["tomo_roftv_tol"] = lambda dx, dy, n: lib.tomo_roftv_tol(0, a(n), P[1], dx, dy, 3, 3, 0.04, 0.005, 3, 0, *tol)
    e["tomo_pdtv_slices"] = lambda dx, dy, n: lib.tomo_pdtv_slices(0, a(n), P[1], dx, dy, 3, *pd, *tol)
    e["tomo_roftv_slices"] = lambda dx, dy, n: lib.tomo_roftv_slices(0, a(n), P[1], dx, dy, 3, 0.04, 0.005, 3, 0, *tol)
    e["tomo_ndf"] = lambda dx, dy, n: lib.tomo_ndf(0, a(n), P[1], dx, dy, 3, 3, 1.0, 2.0, 0.05, 0, 3, 0.0, None, None, None)
    e["tomo_diff4th"] = lambda dx, dy, n: lib.tomo_diff4th(0, a(n), P[1], dx, dy, 3, 3, 1.0, 2.0, 0.005, 3, 0.0, None, None, None)
    e["tomo_llt_rof"] = lambda dx, dy, n: lib.tomo_llt_rof(0, a(n), P[1], dx, dy, 3, 3, 0.3, 0.1, 0.005, 3, 0.0, None, None, None)
    e["tomo_tgv"] = lambda dx, dy, n: lib.tomo_tgv(0, a(n), P[1], dx, dy, 3, 3, 1.0, 1.0, 2.0, 0.25, 0.25, 3, 0.0, None, None, None)
    e["tomo_pdhg_tv_dual"] = lambda dx, dy, n: lib.tomo_pdhg_tv_dual(0, a(n), P[1], P[2], P[3], dx, dy, 3, 3, 0.25, 0.5, 0, None)
    e["tomo_pdhg_primal"] = lambda dx, dy, n: lib.tomo_pdhg_primal(0, a(n), P[1], P[2], P[3], P[4], P[5], dx, dy, 3, 3, 0.25, 0, None)
    e["tomo_pdhg_primal_diag"] = lambda dx, dy, n: lib.tomo_pdhg_primal_diag(0, a(n), P[1], P[2], P[3], P[4], P[5], P[6], dx, dy, 3, 3, 0, None)
    e["tomo_spdhg_tv_dual"] = lambda dx, dy, n: lib.tomo_spdhg_tv_dual(0, a(n), P[1], P[2], P[3], P[4], P[5], P[6], dx, dy, 3, 3, 0.25, 0.5, 0, None)
    e["tomo_spdhg_tv_primal"] = lambda dx, dy, n: lib.tomo_spdhg_tv_primal(0, a(n), P[1], P[2], P[3], P[4], dx, dy, 3, 3, 0.25, 2.0, 0, None)
    for name, more in (("ndf", (1.0, 2.0, 0.05, 0)), ("diff4th", (1.0, 2.0, 0.005)), ("llt_rof", (0.3, 0.1, 0.005))):
        e[f"tomo_{name}_iter_slab_range"] = (lambda dx, dy, n, name=name, more=more:
                                             getattr(lib, f"tomo_{name}_iter_slab_range")(0, a(n), P[1], P[2], dx, dy, 4, 0, 0, 0, 4, *more, None))
    return e


def _slab_tv():
    """the PD_TV and ROF_TV slab entries check no pointer on the host: their next check is the plane range (or none)"""
    from tomobar_amd import _lib
    lib = _lib.lib()
    three = (C.c_void_p * 3)(0x9000, 0xa000, 0xb000)
    multi = lambda dx, dy, z0=0, z1=4: lib.tomo_pdtv_multi_slab_range(0, P[0], P[1], P[2], three, three, dx, dy, 4, 0, 0, z0, z1, 3,   # noqa: E731
                                                                      0.25, 0.25, 0.1, 1.0, 0, 0, 0, None)
    single = lambda dx, dy: lib.tomo_pdtv_iter_slab(0, P[0], P[1], P[2], three, three, dx, dy, 4, 0, 0,   # noqa: E731
                                                    0.25, 0.25, 0.1, 1.0, 0, 0, 0, None)
    rof = lambda dx, dy, z0=0, z1=4: lib.tomo_roftv_iter_slab_range(0, P[0], P[1], P[2], dx, dy, 4, 0, 0, z0, z1, 0.04, 0.005, 0, None)  # noqa: E731
    return multi, single, rof


def _refused(rc, text):
    from tomobar_amd import _lib
    assert rc == _lib.E_INVALID, rc
    with pytest.raises(ValueError) as err:
        _lib.check(rc)
    assert text in str(err.value), (text, str(err.value))


@pytest.mark.parametrize("name", ["tomo_pdtv", "tomo_pdtv_tol", "tomo_roftv", "tomo_roftv_tol", "tomo_pdtv_slices", "tomo_roftv_slices",
                                  "tomo_ndf", "tomo_diff4th", "tomo_llt_rof", "tomo_tgv", "tomo_pdhg_tv_dual", "tomo_pdhg_primal",
                                  "tomo_pdhg_primal_diag", "tomo_spdhg_tv_dual", "tomo_spdhg_tv_primal", "tomo_ndf_iter_slab_range",
                                  "tomo_diff4th_iter_slab_range", "tomo_llt_rof_iter_slab_range"])
def test_a_plane_of_2_to_the_29_is_refused_and_the_largest_below_it_is_not(name):
    call = _entries()[name]
    dy, dx = LI.FLAT_REFUSED
    _refused(call(dx, dy, False), f"a plane of {dx} x {dy} {PLANE_LIMIT}")
    _refused(call(dx, dy, True), PLANE_LIMIT)          # the plane is looked at before the pointers
    _refused(call(2 ** 15, 2 ** 14, False), PLANE_LIMIT)   # 2^29 exactly
    dy, dx = LI.FLAT
    _refused(call(dx, dy, True), "NULL data pointer")  # ... and the largest accepted plane gets as far as the next check


def test_the_tv_slab_entries_refuse_the_plane():
    multi, single, rof = _slab_tv()
    dy, dx = LI.FLAT_REFUSED
    for call in (multi, single, rof):
        _refused(call(dx, dy), f"a plane of {dx} x {dy} {PLANE_LIMIT}")
        _refused(call(2 ** 15, 2 ** 14), PLANE_LIMIT)
    dy, dx = LI.FLAT
    _refused(multi(dx, dy, z0=3, z1=2), "bad output plane range")
    _refused(rof(dx, dy, z0=3, z1=2), "bad output plane range")
    # (tomo_pdtv_iter_slab has no check behind the plane's: an accepted plane would reach the device, so it is not called)


def _wavelet_calls():
    from tomobar_amd import _lib
    lib = _lib.lib()
    return {"tomo_wavelet_shrink": lambda dx, dy, n: lib.tomo_wavelet_shrink(0, NUL if n else P[0], P[1], None, dx, dy, 3, 3, 0.5, None),
            "tomo_wavelet_forward": lambda dx, dy, n: lib.tomo_wavelet_forward(0, NUL if n else P[0], P[1], dx, dy, 3, 3, 0.5, None),
            "tomo_wavelet_inverse": lambda dx, dy, n: lib.tomo_wavelet_inverse(0, NUL if n else P[0], P[1], None, dx, dy, 3, 3, None)}


@pytest.mark.parametrize("name", ["tomo_wavelet_shrink", "tomo_wavelet_forward", "tomo_wavelet_inverse"])
def test_the_wavelets_refuse_a_slice_of_2_to_the_30(name):
    call = _wavelet_calls()[name]
    _refused(call(2 ** 15, 2 ** 15, False), "a slice of 32768 x 32768 is too large")
    _refused(call(2 ** 15, 2 ** 15, True), "is too large")
    _refused(call(2 ** 15 + 1, 2 ** 15, False), "is too large")
    _refused(call(2 ** 15, 2 ** 15 - 1, True), "NULL data pointer")    # 2^30 - 2^15: accepted, on to the next check
    dy, dx = LI.FLAT
    _refused(call(dx, dy, True), "NULL data pointer")


@pytest.mark.parametrize("name", ["tomo_patch_select", "tomo_nltv"])
def test_nltv_refuses_an_extent_above_65535(name):
    from tomobar_amd import _lib
    lib = _lib.lib()
    if name == "tomo_patch_select":
        call = lambda dx, dy, n: lib.tomo_patch_select(0, NUL if n else P[0], P[1], P[2], P[3], dx, dy, 3, 3, 3, 1, 8, 0.5, None)   # noqa: E731
        nxt = "NULL data pointer"
    else:
        call = lambda dx, dy, n: lib.tomo_nltv(0, P[0], P[1], NUL if n else P[2], P[3], P[4], dx, dy, 3, 3, 8, 0.5, 3, 0.0,   # noqa: E731
                                               None, None, None)
        nxt = "NULL table pointer"
    limit = "exceeds the 65535 a 16-bit index table addresses"
    _refused(call(65536, 4, False), f"a slice of 65536 x 4 {limit}")
    _refused(call(4, 65536, True), f"a slice of 4 x 65536 {limit}")
    _refused(call(65535, 4, True), nxt)
    _refused(call(4, 65535, True), nxt)
    dy, dx = LI.FLAT
    _refused(call(dx, dy, True), nxt)
