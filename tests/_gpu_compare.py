"""TEST INFRASTRUCTURE: how the PDHG and SPDHG GPU tests bring a device array to the host and hold it to an oracle's array bit
for bit.  Nothing here touches a GPU on import."""
import numpy as np


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        raise AssertionError((what, f"{len(bad)} of {got.size} values differ, first at {tuple(bad[0])}",
                              float(np.abs(got.astype(np.float64) - want).max())))
