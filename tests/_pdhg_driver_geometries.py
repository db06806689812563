"""TEST INFRASTRUCTURE: the geometries the PDHG and SPDHG driver tests run on (tests/test_gpu_pdhg.py, _tgv, _stripe and
tests/test_gpu_spdhg.py build their `geometries` fixture here): the 4 x 24 x 24 golden case (plain, with a padded detector,
one plane of it) and a 5 x 48 x 48 case of two boxes with Gaussian noise.  Nothing here touches a GPU on import."""
import os

import numpy as np

import _matched_bp_oracle as M

LABELS = ["detY", "angles", "detX"]


class Geometry:
    def __init__(self, nz, n, angles, sino, L_A, pad=0):
        self.nz, self.n, self.angles, self.sino, self.L_A, self.pad = nz, n, angles, sino, float(L_A), pad
        self.size = n + 2 * pad        # the reconstruction grid grows with the padded detector

    def tools(self, **kw):
        from tomobar_amd.methodsIR_CuPy import RecToolsIRCuPy
        return RecToolsIRCuPy(self.n, self.pad, self.nz if self.nz > 1 else None, 0.0, self.angles, self.n, 0,
                              kw.pop("OS_number", None), adjoint=kw.pop("adjoint", "matched"))

    def projector(self):
        return M.MatchedProjector(self.nz, self.size, self.size, self.angles, 0.0)

    def data(self, **kw):
        import torch
        return dict({"projection_data": torch.from_numpy(self.sino.copy()).cuda(), "data_axes_labels_order": list(LABELS)}, **kw)


def build(oracle, golden_dir, Geometry=Geometry):
    """name -> Geometry (or the subclass given); `oracle`, `golden_dir`: the fixtures of tests/conftest.py"""
    gold = np.load(os.path.join(golden_dir, "outer_golden.npz"))
    a48 = np.linspace(0.0, np.pi, 23, endpoint=False)
    vol = np.zeros((5, 48, 48), np.float32)
    vol[:, 12:30, 16:36] = 1.0
    vol[2:, 20:26, 18:30] = 2.5
    rng = np.random.default_rng(43)
    s48 = oracle.Projector(5, 48, 48, a48).fp(vol)
    s48 = (s48 + 0.5 * rng.standard_normal(s48.shape)).astype(np.float32)
    gsino = np.ascontiguousarray(gold["sino"], np.float32)
    out = {"golden": Geometry(4, 24, gold["angles"], gsino, gold["L_full"]),
           "golden_pad": Geometry(4, 24, gold["angles"], gsino, gold["L_full"], pad=4),
           "golden_2d": Geometry(1, 24, gold["angles"], np.ascontiguousarray(gsino[1:2]), gold["L_full"]),
           "n48": Geometry(5, 48, a48, s48, 1500.0)}
    for g in out.values():
        g.sino.setflags(write=False)
    return out


def x0(shape):
    return (0.05 * np.random.default_rng(47).random(shape)).astype(np.float32)
