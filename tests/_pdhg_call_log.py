"""TEST INFRASTRUCTURE: ``RecToolsIRCuPy.PDHG`` on CPU tensors with every projector call and launch replaced by a recorder, for
the tests that pin the driver's sequence of calls without a GPU (tests/test_pdhg_diag_oracle.py,
tests/test_pdhg_stripe_surface.py).  Nothing here touches a GPU."""

VOL, SINO = (2, 4, 4), (2, 3, 4)
LAUNCHES = ("pdhg_sino_dual", "pdhg_tv_dual", "pdhg_primal", "pdhg_sino_dual_diag", "pdhg_primal_diag")


def recording_driver(monkeypatch, fill_shape=False, more_ops=()):
    """(a RecToolsIRCuPy whose projector and launches are recorders, the log of their calls).  `fill_shape`: a fill is logged with
    the shape of its array behind the value; `more_ops`: further names of ``ops`` to record beside LAUNCHES."""
    import torch
    from tomobar_amd import methodsIR_CuPy as M
    log = []

    class Tools:
        device_index, slab, detectors_x_pad, adjoint, _device = 0, None, 0, "matched", "cpu"
        vol_geom = {"GridSliceCount": VOL[0], "GridRowCount": VOL[1], "GridColCount": VOL[2]}
        def vol_shape(self): return VOL
        def sino_shape(self, sub): return SINO
        def invalidate(self): log.append("A.invalidate")
        def set_residual_layout(self, layout): log.append(f"A.set_residual_layout {layout}")
        def set_volume_layout(self, layout): log.append(f"A.set_volume_layout {layout}")
        def forward(self, vol, sub, out=None): log.append("A.forward")
        def backward(self, sino, sub, out=None): log.append("A.backward")

    def work_arrays(shape, device, tv=True, tau=False):
        log.append("pdhg_work_arrays" + (" tau" if tau else ""))
        new = lambda: torch.zeros(shape)   # noqa: E731
        q = [new() for _ in range(3 if tv else 0)]
        return (new(), new(), q, new(), None) if tau else (new(), new(), q, None)

    def fill(x, value):
        log.append(f"fill {float(value)} {tuple(x.shape)}" if fill_shape else f"fill {float(value)}")

    monkeypatch.setattr(M.ops, "to_device", lambda x, index: x)
    monkeypatch.setattr(M.ops, "fill", fill)
    monkeypatch.setattr(M.ops, "pdhg_work_arrays", work_arrays)
    for name in LAUNCHES + tuple(more_ops):
        monkeypatch.setattr(M.ops, name, lambda *args, _name=name: log.append(_name))

    def no_power_method(self, data):
        raise AssertionError("the power method ran")

    monkeypatch.setattr(M.RecToolsIRCuPy, "powermethod", no_power_method)
    rt = M.RecToolsIRCuPy.__new__(M.RecToolsIRCuPy)
    rt.__dict__.update(Atools=Tools(), _slab=None, _OS_number=1, _objsize_user_given=None, last_run=None)
    return rt, log
