"""TEST INFRASTRUCTURE: guard bands round every array a kernel reads or writes.  `guarded` places an array in the middle of
a larger allocation whose every other element holds one fixed bit pattern; `intact()` says afterwards whether a store landed
outside the array (and where), and -- the pattern of the float types being a NaN -- a load from outside the array shows up
in the values the kernel returns.  tests/test_guarded.py proves the helper on the CPU; tests/_march_gpu.py,
tests/test_gpu_pdhg.py, tests/test_gpu_spdhg.py, tests/test_gpu_bp_epilogues.py and tests/test_gpu_guards.py use it on the
MI355X.  Nothing here touches a GPU on import.

The width of the band on each side, in elements, is

    max(1024, numel + 16 * plane)         plane = the product of the last two dimensions, 0 for a 1-D array

  1024      what one workgroup of 256 threads covers with one float4 access each: a streaming kernel whose tail mask is
            wrong by a whole block still lands in the band (CITES: EW_BLOCK of glue_kernels.hip, STREAM_BLOCK of
            pdhg_kernels.hip, the float4 index `i4` of ew_vec4);
  16 plane  the deepest output tile in the tree is 16 planes: 4 * BB_ZQ planes of the voxel-driven back projector's brick
            (bp_brick.inl, BB_ZQ = 4) and 4 * MB_ZQ of the matched one (bp_matched.hip, MB_ZQ = 4); the z-marching
            regularisers write one plane per step;
  numel     a whole-array offset error (the wrong one of two arrays, an index one array too far) at the tiny shapes the
            tests use.

A deeper tile raises the rule; nothing lowers it.  tests/test_guarded.py requires every text of CITES to be in its file
still."""
import collections

import numpy as np

# (file under tomobar_amd/csrc, text the number was read from)
CITES = [
    ("glue_kernels.hip", "constexpr int EW_BLOCK = 256;"),
    ("glue_kernels.hip", "__global__ __launch_bounds__(EW_BLOCK) void ew_vec4("),
    ("pdhg_kernels.hip", "constexpr int STREAM_BLOCK = 256;"),
    ("bp_brick.inl", "constexpr int BB_TX = 32, BB_TY = 16, BB_ZQ = 4, BB_AB = 8;"),
    ("bp_brick.inl", "const int z0 = zb * (4 * BB_ZQ);"),
    ("bp_matched.hip", "constexpr int MB_TX = 32, MB_TY = 16, MB_ZQ = 4, MB_AB = 8;"),
    ("bp_matched.hip", "const int z0 = zb * (4 * MB_ZQ);"),
]

WORKGROUP_FLOAT4 = 256 * 4     # EW_BLOCK / STREAM_BLOCK threads, one float4 each
DEEPEST_TILE_PLANES = 4 * 4    # 4 * BB_ZQ = 4 * MB_ZQ

# the band's bit pattern by element size: a quiet NaN with a payload for the 32-bit types (float32 reads it as NaN, int32
# as a number no index table holds), fixed non-zero patterns for uint16 tables and byte buffers
PATTERN = {4: 0x7FC0BEEF, 2: 0xBEEF, 1: 0xA5}
_UINT = {4: np.uint32, 2: np.uint16, 1: np.uint8}


def band_width(shape, planes=None):
    """elements of band on each side of a view of `shape`; `planes` replaces the product of the last two dimensions for a
    flat buffer whose size an API fixes (a residual of tomo_ctx_residual_elems floats is 1-D, its planes are not)"""
    shape = tuple(int(s) for s in shape)
    numel = int(np.prod(shape, dtype=np.int64))
    plane = (shape[-1] * shape[-2] if len(shape) >= 2 else 0) if planes is None else int(planes)
    return max(WORKGROUP_FLOAT4, numel + DEEPEST_TILE_PLANES * plane)


class Intact(collections.namedtuple("Intact", "ok offset")):
    """(ok, offset): `offset` is the first damaged element relative to the view's first (negative: before the view; from
    the view's size on: after it), None when ok.  Truth value = ok, so `assert g.intact()` works."""
    __slots__ = ()

    def __bool__(self):
        return bool(self.ok)


class Guarded:
    """what `guarded` returns.  `.view`: the contiguous tensor of the requested shape; `.buf`: the whole allocation in the
    view's element type; `.dtype`: the numpy type of both."""

    def __init__(self, raw, start, numel, shape, np_dtype, given):
        import torch
        self._raw, self._start, self._numel, self._given = raw, start, numel, given
        self.dtype = np.dtype(np_dtype)
        tdtype = getattr(torch, self.dtype.name)
        self.buf = raw.view(tdtype)
        isz = self.dtype.itemsize
        self.view = raw[start * isz:(start + numel) * isz].view(tdtype).view(shape)
        assert self.view.is_contiguous()

    # -------------------------------------------------------------------------------- reading back
    def _host_bytes(self):
        if self._raw.is_cuda:
            import torch
            torch.cuda.synchronize(self._raw.device)
        return self._raw.detach().cpu().numpy()

    def host(self):
        """the view on the host, in its own dtype"""
        if self.view.is_cuda:
            import torch
            torch.cuda.synchronize(self.view.device)
        return self.view.detach().cpu().numpy().copy()

    def intact(self):
        """both bands still hold the pattern, compared as integers"""
        isz = self.dtype.itemsize
        words = self._host_bytes().view(_UINT[isz])
        pat = _UINT[isz](PATTERN[isz])
        lo = np.flatnonzero(words[:self._start] != pat)
        if lo.size:
            return Intact(False, int(lo[0]) - self._start)
        hi = np.flatnonzero(words[self._start + self._numel:] != pat)
        if hi.size:
            return Intact(False, self._numel + int(hi[0]))
        return Intact(True, None)

    def unchanged(self):
        """the view holds the bits it was given (a read-only input after the call)"""
        assert self._given is not None, "made from a shape: there is nothing to compare with"
        isz = self.dtype.itemsize
        return bool(np.array_equal(self.host().view(_UINT[isz]), self._given.view(_UINT[isz])))

    def check(self, what="", read_only=False):
        res = self.intact()
        assert res.ok, (what, "a guard band was written", res.offset, tuple(self.view.shape))
        if read_only:
            assert self.unchanged(), (what, "a read-only input was written")


def guarded(a_or_shape, *, dtype=np.float32, fill=None, shift=0, planes=None, device="cuda"):
    """`a_or_shape`: an array (copied into the view as `dtype`; an integer array keeps its own type) or a shape (the view
    is filled with `fill`; default NaN for float32, so an element the kernel never wrote shows; 0 for the integer types).  `shift` = k in 0..3: the view starts 4 k bytes past a 16-byte
    boundary.  `planes`: see band_width.  Returns a Guarded: .view, .buf, .intact(), .host(), .unchanged(), .check()."""
    import torch
    given = None
    if isinstance(a_or_shape, np.ndarray):
        if dtype is np.float32 and a_or_shape.dtype.kind in "iu":   # an index table or a byte buffer keeps its type
            dtype = a_or_shape.dtype
        given = np.ascontiguousarray(a_or_shape, dtype=dtype)
        shape = given.shape
    else:
        shape = (int(a_or_shape),) if np.isscalar(a_or_shape) else tuple(int(s) for s in a_or_shape)
    dt = np.dtype(dtype)
    isz = dt.itemsize
    assert isz in PATTERN, dt
    assert shift in (0, 1, 2, 3), shift
    numel = int(np.prod(shape, dtype=np.int64))
    width = band_width(shape, planes)
    # low band >= width, rounded up so that the view can start on a 16-byte boundary wherever the allocation starts
    total = (2 * width + numel) * isz + 16 + 4 * shift + 16
    total = (total + 15) // 16 * 16
    raw = torch.empty(total, dtype=torch.uint8, device=device)
    base = raw.data_ptr()
    assert base % 4 == 0, base
    start_byte = width * isz
    start_byte += (-(base + start_byte)) % 16 + 4 * shift
    assert start_byte % isz == 0
    start = start_byte // isz
    image = np.full(total // isz, PATTERN[isz], dtype=_UINT[isz])
    inner = image[start:start + numel].view(dt)
    if given is not None:
        inner[:] = given.ravel()
    else:
        inner[:] = (np.nan if dt.kind == "f" else 0) if fill is None else fill
    raw.copy_(torch.from_numpy(image.view(np.uint8)))
    g = Guarded(raw, start, numel, shape, dt, given)
    assert g.view.data_ptr() % 16 == 4 * shift, (g.view.data_ptr(), shift)
    assert start >= width and total // isz - (start + numel) >= width, (start, width)
    return g
