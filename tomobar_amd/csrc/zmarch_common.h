// What the z-march operators (tgv_kernels.hip, ndf_kernels.hip, diff4th_kernels.hip, llt_rof_kernels.hip, pdhg_kernels.hip)
// share: the device helpers of a plane march, its launch grid, the layout of a work array, the early-stopping check and the
// host driver of an explicit time march.  Everything here is internal to the including translation unit (anonymous namespace).
//
// tv_kernels.hip does not include this header and keeps its own PlaneIO, zmarch_grid, tv_skew and tolerance rule: its
// bytes are pinned by hash (profiles/pmc_traffic.json is keyed to them), so the copy there cannot be replaced by this one.
#pragma once
#include "tomo_common.h"
#include <cmath>

namespace {

// one-lane wave shifts (gfx9 DPP, a single VALU move); the lane shifted in at the wave's end is a halo lane's, never consumed
__device__ __forceinline__ float wave_prev(float v)  // lane i <- lane i-1
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x138 /*wave_shr:1*/, 0xf, 0xf, true));
}
__device__ __forceinline__ float wave_next(float v)  // lane i <- lane i+1
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x130 /*wave_shl:1*/, 0xf, 0xf, true));
}

// Plane-relative buffer addressing (see PlaneIO in tv_kernels.hip): `xo` = byte offset of the lane's column inside a row
// (VGPR), `ro` = byte offset of the row inside the plane (wave-uniform, the instruction's soffset).  One descriptor per
// (array, plane); callers clamp column, row and plane, so `ro + xo` always lies inside the plane.
struct PlaneIO {
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

// The launch grid of a z-march (zmarch_grid of tv_kernels.hip, with ROF_TV's targets): a workgroup of wx x wy waves covers
// wx tiles of `tile_x` columns by wy * ry rows; the `nout` output planes of a 3D volume are cut into z-chunks, enough for
// 32 waves on each of the chip's 256 x 4 SIMDs but none shorter than 16 planes; workgroups are numbered so that each of
// the 8 XCDs gets `tiles_per_xcd` xy tiles of every chunk.  `op` names the operator in the error message.
struct ZmarchGrid {
    int gx, gy, tiles_per_xcd, zchunk;
    long blocks;
};
static int zmarch_grid(ZmarchGrid &g, const char *op, int dx, int dy, int nout, int tile_x, int wx, int wy, int ry, bool chunked)
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
    if (g.blocks > 0x7fffffffL) return tomo_fail(TOMO_E_INVALID, "volume too large for one %s launch", op);
    return TOMO_OK;
}

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// bytes between consecutive work arrays beyond the plain packing (tv_skew of tv_kernels.hip: equal-sized arrays laid end to
// end put the same voxel of every array on the same HBM channel and bank)
constexpr size_t WORK_SKEW = 69888;

// what one work array of `nvox` floats takes in the placed TV arena
inline size_t work_array_bytes(size_t nvox) { return align_up(nvox * sizeof(float), 256) + WORK_SKEW; }

// ---- the early-stopping rule of tomo_pdtv_tol / tomo_roftv_tol (include/tomo_mi355x.h)
constexpr int TOL_INTERVAL = 6, TOL_MIN_SAVED = 3;

// The snapshot U_{n-6} of a run that can stop early (else `snap` stays null): a block of its own, the TV arena keeps its
// size and placement.
static int tol_snapshot(int device, hipStream_t st, double tol, int iters, size_t nvox, float *&snap)
{
    snap = nullptr;
    if (tol > 0.0 && iters >= TOL_INTERVAL + TOL_MIN_SAVED) {
        void *p = nullptr;
        int rc = tomo_arena_get(device, st, ARENA_TVSNAP, nvox * sizeof(float), &p);
        if (rc != TOMO_OK) return rc;
        snap = (float *)p;
    }
    return TOMO_OK;
}

// is iterate n of `iters` a check point?
inline bool tol_due(const float *snap, int n, int iters) { return snap != nullptr && n % TOL_INTERVAL == 0 && iters - n >= TOL_MIN_SAVED; }

// The check at check point n on the iterate `cur`: the first one reads the caller's input as the reference and only writes
// the snapshot; later ones compare with the snapshot and refresh it in the same pass.  `d` is the relative change, `stop`
// whether it is below the tolerance.
struct TolCheck {
    bool stop;
    double d;
};
static int tol_check(TolCheck &c, int n, const float *cur, const float *in_dev, float *snap, size_t nvox, double tol, hipStream_t st)
{
    double s[2];
    int rc = tomo_rel_change(cur, n == TOL_INTERVAL ? in_dev : snap, snap, nvox, s, st);
    if (rc != TOMO_OK) return rc;
    c.d = s[0] == 0.0 ? 0.0 : (s[1] == 0.0 ? INFINITY : sqrt(s[0] / s[1]));
    c.stop = c.d < tol;
    return TOMO_OK;
}

// ---- explicit time marching (NDF, Diff4th, LLT_ROF): one launch per iteration that reads neighbours of the field it
// writes, so U is ping-ponged between the caller's output array and ONE work array in the placed TV arena.
inline size_t march_scratch_bytes(int dx, int dy, int dz, int nd)
{
    if (nd == 2) dz = 1;
    return work_array_bytes((size_t)dx * dy * dz);   // the one ping-pong partner of the output array
}

// The whole-volume entry point behind tomo_ndf / tomo_diff4th / tomo_llt_rof once the operator's own parameters are
// checked: `launch(u_in, u_out)` runs one iteration and returns a TOMO_* code, `op` names the operator in messages.
template <typename Launch>
static int march_run(const char *op, int device, const float *in_dev, float *out_dev, int dx, int dy, int dz, int nd, int iters,
                     double tol, int *iters_done, double *last_rel_change, void *stream, Launch launch)
{
    TOMO_REQUIRE(device >= 0, "The gpu_device must be a positive integer or zero");
    TOMO_REQUIRE(nd == 2 || nd == 3, "2D or 3D arrays must be provided only");
    if (nd == 2) dz = 1;
    TOMO_REQUIRE(dx >= 1 && dy >= 1 && dz >= 1, "%s needs every dimension >= 1", op);
    TOMO_REQUIRE(iters >= 0, "%s: the number of iterations must not be negative", op);
    TOMO_REQUIRE(tol >= 0.0 && std::isfinite(tol), "the tolerance must be a finite number >= 0");
    TOMO_REQUIRE((size_t)dx * (size_t)dy < ((size_t)1 << 29), "a plane of %d x %d exceeds the 2 GiB a buffer descriptor of the TV kernels addresses", dx, dy);
    TOMO_REQUIRE(in_dev && out_dev, "NULL data pointer");
    TOMO_REQUIRE(in_dev != out_dev, "%s: the output must not alias the input (the iterations ping-pong through the output array)", op);
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
        rc = tomo_arena_get(device, st, ARENA_TV, march_scratch_bytes(dx, dy, dz, nd), &base, true);
        if (rc != TOMO_OK) return rc;
        work = (float *)base;
    }
    float *snap;
    rc = tol_snapshot(device, st, tol, iters, nvox, snap);
    if (rc != TOMO_OK) return rc;

    // iterate n lives in the output array when iters - n is even, else in the work array: the last one is the caller's
    auto home = [&](int n) { return (iters - n) % 2 == 0 ? out_dev : work; };
    for (int n = 1; n <= iters; ++n) {
        float *cur = home(n);
        rc = launch(n == 1 ? in_dev : home(n - 1), cur);
        if (rc != TOMO_OK) return rc;
        if (!tol_due(snap, n, iters)) continue;
        TolCheck c;
        rc = tol_check(c, n, cur, in_dev, snap, nvox, tol, st);
        if (rc != TOMO_OK) return rc;
        if (last_rel_change) *last_rel_change = c.d;
        if (c.stop) {
            if (iters_done) *iters_done = n;
            if (cur != out_dev)
                TOMO_HIP(hipMemcpyAsync(out_dev, cur, nvox * sizeof(float), hipMemcpyDeviceToDevice, st));
            return TOMO_OK;
        }
    }
    return TOMO_OK;
}

// The common part of the tomo_*_iter_slab_range entry points, which run one iteration on arrays that carry `ghost` planes
// per interior boundary: the argument checks and the device.  `launch()` runs when there are output planes.
template <typename Launch>
static int march_slab_range(const char *op, int ghost, int device, const float *in_dev, const float *u_in_dev, float *u_out_dev,
                            int dx, int dy, int nz_local, int lo_planes, int hi_planes, int z_begin, int z_end, Launch launch)
{
    TOMO_REQUIRE(device >= 0 && dx >= 1 && dy >= 1 && nz_local >= 1, "bad slab arguments");
    TOMO_REQUIRE((size_t)dx * (size_t)dy < ((size_t)1 << 29), "a plane of %d x %d exceeds the 2 GiB a buffer descriptor of the TV kernels addresses", dx, dy);
    TOMO_REQUIRE(z_begin >= 0 && z_begin <= z_end && z_end <= nz_local, "bad output plane range [%d, %d)", z_begin, z_end);
    TOMO_REQUIRE((lo_planes == 0 || lo_planes == ghost) && (hi_planes == 0 || hi_planes == ghost),
                 "%s slab needs 0 or %d ghost plane%s below and 0 or %d above", op, ghost, ghost == 1 ? "" : "s", ghost);
    TOMO_REQUIRE(in_dev && u_in_dev && u_out_dev, "NULL data pointer");
    TOMO_REQUIRE(u_in_dev != u_out_dev && in_dev != u_out_dev, "%s slab: the output array must not alias an array the launch reads", op);
    if (z_begin == z_end) return TOMO_OK;
    TOMO_ON_DEVICE(device);
    return launch();
}

}  // namespace
