// LLT_ROF regulariser for gfx950: the combined first- and second-order model (ROF total variation plus the fourth-order
// Lysaker-Lundervold-Tai term), explicit in time,
//     U' = U - tau ((lambda_llt B - lambda_rof V) + (U - f)),   U^0 = f,
// with V the divergence of the ROF flux R = grad U / sqrt(|grad U|^2 + eps) (forward differences) and B the sum over the
// axes of the second difference of the LLT flux E_d = h_d / (|h_d| + eps), h_d the second difference of U along d.  The
// reference's dicts_check names LLT_ROF next to time_marching_step (tomobar/supp/dicts.py:173, "ROF_TV, LLT_ROF, NDF,
// Diff4th") but nothing in its tree implements it: what is computed is the algorithm stated in docs/kernels/llt_rof.md,
// formula-level parity, unpinned -- tests/_llt_rof_oracle.py restates it in numpy and the kernel reproduces its float32
// form bit for bit (one rounding per operation in the stated order, no FMA contraction: -ffp-contract=off and no fmaf
// here; / and sqrtf are the compiler's correctly rounded ones).
//
// One launch per iteration with both stages fused, a plane march on the skeleton of diff4th_zmarch.inl
// (llt_rof_zmarch.inl): the six flux fields stay in registers, U is read once (plus halos and the seam planes of a
// z-chunk), f read once, U' written once -- 12 B per voxel and iteration.  The launch reads neighbours of the field it
// writes, so U is ping-ponged between the caller's output array and ONE work array in the placed TV arena; the first
// iteration reads the input itself as U^0 and the last one writes the output array.  The same kernel serves the z-slab
// form (tomo_llt_rof_iter_slab_range): arrays with two ghost planes per interior boundary.
//
// tv_kernels.hip is pinned by hash (profiles/pmc_traffic.json), so the few host helpers this file shares with it in spirit --
// the z-march grid, the array skew, the tolerance rule -- are restated here, as ndf_kernels.hip and diff4th_kernels.hip
// restate them.
#include "tomo_common.h"
#include <cmath>

namespace {

// one-lane wave shifts (gfx9 DPP, a single VALU move); the lane shifted in at the wave's end is a halo lane's, never consumed
__device__ __forceinline__ float lr_prev(float v)  // lane i <- lane i-1
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x138 /*wave_shr:1*/, 0xf, 0xf, true));
}
__device__ __forceinline__ float lr_next(float v)  // lane i <- lane i+1
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x130 /*wave_shl:1*/, 0xf, 0xf, true));
}

// Plane-relative buffer addressing (TgvPlane of tgv_kernels.hip): `xo` = byte offset of the lane's column inside a row
// (VGPR), `ro` = byte offset of the row inside the plane (wave-uniform, the instruction's soffset).  One descriptor per
// (array, plane); callers clamp column, row and plane, so `ro + xo` always lies inside the plane.
struct LrPlane {
    int bytes;  // size of one float plane in bytes
    __device__ __forceinline__ __amdgpu_buffer_rsrc_t rs(const void *plane) const
    {
        return __builtin_amdgcn_make_buffer_rsrc((void *)plane, 0, bytes, 0x00020000);
    }
    __device__ __forceinline__ float ld(const float *plane, unsigned xo, int ro) const
    {
        return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs(plane), (int)xo, ro, 0));
    }
    __device__ __forceinline__ void st(float *plane, unsigned xo, int ro, float v) const
    {
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v), rs(plane), (int)xo, ro, 0);
    }
};

// One iteration on arrays of `planes` planes [dy][dx]: the output planes [out_begin, out_end) of `u_out` are written.  A
// plane of the arrays has a z-neighbour wherever the arrays hold one: the whole volume is planes = dz, a z-slab carries
// its ghost planes inside `planes` (the z index is clamped only at the global faces).
struct LrArgs {
    const float *f;      // the input (read at the output voxels only)
    const float *u_in;   // the current iterate (the input itself in the first iteration)
    float *u_out;
    int dx, dy, planes, out_begin, out_end;
    float lambda_rof, lambda_llt, tau;
};

// The launch grid of a z-march (tgv_grid of tgv_kernels.hip): a workgroup of wx x wy waves covers wx tiles of `tile_x`
// columns by wy * ry rows; 3D volumes are cut into z-chunks, enough for 32 waves on each of the chip's 256 x 4 SIMDs but
// none shorter than 16 planes; workgroups are numbered so that each of the 8 XCDs gets `tiles_per_xcd` xy tiles of every
// chunk.
struct LrGrid {
    int gx, gy, tiles_per_xcd, zchunk;
    long blocks;
};
static int lr_grid(LrGrid &g, int dx, int dy, int nout, int tile_x, int wx, int wy, int ry, bool chunked)
{
    constexpr long want_per_simd = 32;
    constexpr int min_planes = 16;
    g.gx = ceil_div(ceil_div(dx, tile_x), wx);
    g.gy = ceil_div(dy, wy * ry);
    g.tiles_per_xcd = ceil_div(g.gx * g.gy, 8);
    int chunks = 1;
    if (chunked) {
        const long waves_xy = (long)g.gx * g.gy * wx * wy;
        chunks = (int)((256L * 4 * want_per_simd + waves_xy - 1) / waves_xy);
        const int max_chunks = ceil_div(nout, min_planes);
        if (chunks > max_chunks) chunks = max_chunks;
        if (chunks < 1) chunks = 1;
    }
    g.zchunk = ceil_div(nout, chunks);
    chunks = ceil_div(nout, g.zchunk);
    g.blocks = 8L * g.tiles_per_xcd * chunks;
    if (g.blocks > 0x7fffffffL) return tomo_fail(TOMO_E_INVALID, "volume too large for one LLT_ROF launch");
    return TOMO_OK;
}

#include "llt_rof_zmarch.inl"

// The only LLT_ROF launch site: 8 rows per lane, 2 x 2 waves (docs/kernels/llt_rof.md, "Choosing RY").
static int lr_launch_iteration(const LrArgs &a, int nd, hipStream_t st)
{
    const int rc = nd == 3 ? lr_zmarch_launch<3, 8, 2, 2>(a, st) : lr_zmarch_launch<2, 8, 2, 2>(a, st);
    if (rc != TOMO_OK) return rc;
    TOMO_LAUNCH_CHECK();
    return TOMO_OK;
}

inline size_t lr_align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// bytes after a work array beyond the plain packing (TGV_SKEW of tgv_kernels.hip)
constexpr size_t LR_SKEW = 69888;

// the early-stopping rule of tomo_pdtv_tol / tomo_roftv_tol (include/tomo_mi355x.h)
constexpr int LR_TOL_INTERVAL = 6, LR_TOL_MIN_SAVED = 3;

}  // namespace

// ------------------------------------------------------------------------------------------ C-ABI
extern "C" size_t tomo_llt_rof_scratch_bytes(int dx, int dy, int dz, int nd)
{
    if (nd == 2) dz = 1;
    return lr_align_up((size_t)dx * dy * dz * sizeof(float), 256) + LR_SKEW;   // the one ping-pong partner of the output array
}

extern "C" int tomo_llt_rof(int device, const float *in_dev, float *out_dev, int dx, int dy, int dz, int nd,
                            float lambda_rof, float lambda_llt, float tau, int iters,
                            double tol, int *iters_done, double *last_rel_change, void *stream)
{
    TOMO_REQUIRE(device >= 0, "The gpu_device must be a positive integer or zero");
    TOMO_REQUIRE(nd == 2 || nd == 3, "2D or 3D arrays must be provided only");
    if (nd == 2) dz = 1;
    TOMO_REQUIRE(dx >= 1 && dy >= 1 && dz >= 1, "LLT_ROF needs every dimension >= 1");
    TOMO_REQUIRE(iters >= 0, "LLT_ROF: the number of iterations must not be negative");
    TOMO_REQUIRE(lambda_rof > 0.0f && lambda_llt > 0.0f && tau > 0.0f, "LLT_ROF: the ROF weight, the LLT weight and the step tau must be positive");
    TOMO_REQUIRE(tol >= 0.0 && std::isfinite(tol), "the tolerance must be a finite number >= 0");
    TOMO_REQUIRE((size_t)dx * (size_t)dy < ((size_t)1 << 29), "a plane of %d x %d exceeds the 2 GiB a buffer descriptor of the TV kernels addresses", dx, dy);
    TOMO_REQUIRE(in_dev && out_dev, "NULL data pointer");
    TOMO_REQUIRE(in_dev != out_dev, "LLT_ROF: the output must not alias the input (the iterations ping-pong through the output array)");
    TOMO_ON_DEVICE(device);
    hipStream_t st = as_stream(stream);
    const size_t nvox = (size_t)dx * dy * dz;
    if (iters_done) *iters_done = iters;
    if (last_rel_change) *last_rel_change = NAN;
    if (iters == 0) {
        TOMO_HIP(hipMemcpyAsync(out_dev, in_dev, nvox * sizeof(float), hipMemcpyDeviceToDevice, st));
        return TOMO_OK;
    }

    float *work = nullptr;   // a single iteration goes from the input straight to the output array
    int rc;
    if (iters > 1) {
        void *base = nullptr;
        rc = tomo_arena_get(device, st, ARENA_TV, tomo_llt_rof_scratch_bytes(dx, dy, dz, nd), &base, true);
        if (rc != TOMO_OK) return rc;
        work = (float *)base;
    }
    float *snap = nullptr;   // U_{n-6}: a block of its own, the TV arena keeps its size and placement
    if (tol > 0.0 && iters >= LR_TOL_INTERVAL + LR_TOL_MIN_SAVED) {
        void *p = nullptr;
        rc = tomo_arena_get(device, st, ARENA_TVSNAP, nvox * sizeof(float), &p);
        if (rc != TOMO_OK) return rc;
        snap = (float *)p;
    }

    LrArgs a;
    a.f = in_dev;
    a.dx = dx; a.dy = dy; a.planes = dz; a.out_begin = 0; a.out_end = dz;
    a.lambda_rof = lambda_rof; a.lambda_llt = lambda_llt; a.tau = tau;
    // iterate n lives in the output array when iters - n is even, else in the work array: the last one is the caller's
    auto home = [&](int n) { return (iters - n) % 2 == 0 ? out_dev : work; };
    for (int n = 1; n <= iters; ++n) {
        a.u_in = n == 1 ? in_dev : home(n - 1);
        a.u_out = home(n);
        rc = lr_launch_iteration(a, nd, st);
        if (rc != TOMO_OK) return rc;
        if (snap == nullptr || n % LR_TOL_INTERVAL != 0 || iters - n < LR_TOL_MIN_SAVED) continue;
        // the first check reads the caller's input as the reference and only writes the snapshot; later ones compare with
        // the snapshot and refresh it in the same pass
        double s[2];
        rc = tomo_rel_change(a.u_out, n == LR_TOL_INTERVAL ? in_dev : snap, snap, nvox, s, st);
        if (rc != TOMO_OK) return rc;
        const double d = s[0] == 0.0 ? 0.0 : (s[1] == 0.0 ? INFINITY : sqrt(s[0] / s[1]));
        if (last_rel_change) *last_rel_change = d;
        if (d < tol) {
            if (iters_done) *iters_done = n;
            if (a.u_out != out_dev)
                TOMO_HIP(hipMemcpyAsync(out_dev, a.u_out, nvox * sizeof(float), hipMemcpyDeviceToDevice, st));
            return TOMO_OK;
        }
    }
    return TOMO_OK;
}

extern "C" int tomo_llt_rof_iter_slab_range(int device, const float *in_dev, const float *u_in_dev, float *u_out_dev,
                                            int dx, int dy, int nz_local, int lo_planes, int hi_planes, int z_begin,
                                            int z_end, float lambda_rof, float lambda_llt, float tau, void *stream)
{
    TOMO_REQUIRE(device >= 0 && dx >= 1 && dy >= 1 && nz_local >= 1, "bad slab arguments");
    TOMO_REQUIRE((size_t)dx * (size_t)dy < ((size_t)1 << 29), "a plane of %d x %d exceeds the 2 GiB a buffer descriptor of the TV kernels addresses", dx, dy);
    TOMO_REQUIRE(z_begin >= 0 && z_begin <= z_end && z_end <= nz_local, "bad output plane range [%d, %d)", z_begin, z_end);
    TOMO_REQUIRE((lo_planes == 0 || lo_planes == 2) && (hi_planes == 0 || hi_planes == 2),
                 "LLT_ROF slab needs 0 or 2 ghost planes below and 0 or 2 above");
    TOMO_REQUIRE(lambda_rof > 0.0f && lambda_llt > 0.0f && tau > 0.0f, "LLT_ROF: the ROF weight, the LLT weight and the step tau must be positive");
    TOMO_REQUIRE(in_dev && u_in_dev && u_out_dev, "NULL data pointer");
    TOMO_REQUIRE(u_in_dev != u_out_dev && in_dev != u_out_dev, "LLT_ROF slab: the output array must not alias an array the launch reads");
    if (z_begin == z_end) return TOMO_OK;
    TOMO_ON_DEVICE(device);
    LrArgs a;
    a.f = in_dev; a.u_in = u_in_dev; a.u_out = u_out_dev;
    a.dx = dx; a.dy = dy; a.planes = lo_planes + nz_local + hi_planes;
    a.out_begin = lo_planes + z_begin; a.out_end = lo_planes + z_end;
    a.lambda_rof = lambda_rof; a.lambda_llt = lambda_llt; a.tau = tau;
    return lr_launch_iteration(a, 3, as_stream(stream));
}
