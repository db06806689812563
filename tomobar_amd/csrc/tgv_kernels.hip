// Second-order total generalised variation (TGV, Bredies-Kunisch-Pock) proximal operator for gfx950:
//     argmin_u 1/2 |u - f|^2 + lambda min_v (alpha1 |grad u - v|_1 + alpha0 |E v|_1)
// by Chambolle-Pock iterations.  There is no reference implementation of it in the tree (the reference took TGV from the
// regularisation toolkit it no longer depends on; its dicts_check still carries the "TGV specific" comment above
// PD_LipschitzConstant, tomobar/supp/dicts.py:176-178): what is computed is the algorithm stated in docs/kernels/tgv.md,
// formula-level parity, unpinned -- tests/_tgv_oracle.py restates it in numpy and the kernels reproduce its float32 form
// bit for bit (one rounding per operation in the stated order, no FMA contraction: -ffp-contract=off and no fmaf here;
// sqrtf and / are the compiler's correctly rounded ones).
//
// Two launches per iteration, both plane marches on the skeleton of rof_zmarch.inl:
//   tgv_dual.inl    steps 1-2: reads U-bar, V-bar (planes z and z+1), updates P, Q in place
//   tgv_primal.inl  steps 3-4: reads P, Q (with -x, -y, -z neighbours), U, V, f; updates U, U-bar, V, V-bar in place
// Each voxel's own P, Q, U, V are read by that voxel only, and the neighbours a launch reads belong to fields it does not
// write, so nothing is ping-ponged.  U lives in the caller's output array, the other 16 (3D) / 10 (2D) fields in the
// placed TV arena.  Algorithmic traffic: 44 floats = 176 B per voxel and iteration in 3D, 28 floats = 112 B in 2D.
//
// tv_kernels.hip is pinned by hash (profiles/pmc_traffic.json), so the few host helpers this file shares with it in spirit --
// the z-march grid, the array skew, the tolerance rule -- are restated here instead of being moved into a common header.
#include "tomo_common.h"
#include <cmath>

namespace {

// one-lane wave shifts (gfx9 DPP, a single VALU move); the lane shifted in at the wave's end is a halo lane's, never consumed
__device__ __forceinline__ float tgv_prev(float v)  // lane i <- lane i-1
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x138 /*wave_shr:1*/, 0xf, 0xf, true));
}
__device__ __forceinline__ float tgv_next(float v)  // lane i <- lane i+1
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x130 /*wave_shl:1*/, 0xf, 0xf, true));
}

// Plane-relative buffer addressing (see PlaneIO in tv_kernels.hip): `xo` = byte offset of the lane's column inside a row
// (VGPR), `ro` = byte offset of the row inside the plane (wave-uniform, the instruction's soffset).  One descriptor per
// (array, plane); callers clamp column and row, so `ro + xo` always lies inside the plane.
struct TgvPlane {
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

// Q components; 2D uses the first three
enum { TQ11 = 0, TQ22 = 1, TQ12 = 2, TQ33 = 3, TQ13 = 4, TQ23 = 5 };

struct TgvArgs {
    const float *f;   // the input
    float *u, *ub;    // U (the caller's output array), U-bar
    float *v[3], *vb[3], *p[3], *q[6];
    int dx, dy, dz;
    float lambda, alpha1, alpha0, tau, sigma;
};

// The launch grid of a z-march (zmarch_grid of tv_kernels.hip, with ROF_TV's targets): a workgroup of wx x wy waves covers
// wx tiles of `tile_x` columns by wy * ry rows; 3D volumes are cut into z-chunks, enough for 32 waves on each of the chip's
// 256 x 4 SIMDs but none shorter than 16 planes; workgroups are numbered so that each of the 8 XCDs gets `tiles_per_xcd`
// xy tiles of every chunk.
struct TgvGrid {
    int gx, gy, tiles_per_xcd, zchunk;
    long blocks;
};
static int tgv_grid(TgvGrid &g, int dx, int dy, int dz, int tile_x, int wx, int wy, int ry, bool chunked)
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
        const int max_chunks = ceil_div(dz, min_planes);
        if (chunks > max_chunks) chunks = max_chunks;
        if (chunks < 1) chunks = 1;
    }
    g.zchunk = ceil_div(dz, chunks);
    chunks = ceil_div(dz, g.zchunk);
    g.blocks = 8L * g.tiles_per_xcd * chunks;
    if (g.blocks > 0x7fffffffL) return tomo_fail(TOMO_E_INVALID, "volume too large for one TGV launch");
    return TOMO_OK;
}

#include "tgv_dual.inl"
#include "tgv_primal.inl"

// The only TGV launch sites: 4 rows per lane, 2 x 2 waves.
static int tgv_launch_iteration(const TgvArgs &a, int nd, hipStream_t st)
{
    int rc = nd == 3 ? tgv_dual_launch<3, 4, 2, 2>(a, st) : tgv_dual_launch<2, 4, 2, 2>(a, st);
    if (rc != TOMO_OK) return rc;
    TOMO_LAUNCH_CHECK();
    rc = nd == 3 ? tgv_primal_launch<3, 4, 2, 2>(a, st) : tgv_primal_launch<2, 4, 2, 2>(a, st);
    if (rc != TOMO_OK) return rc;
    TOMO_LAUNCH_CHECK();
    return TOMO_OK;
}

inline size_t tgv_align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// bytes between consecutive work arrays beyond the plain packing (tv_skew of tv_kernels.hip: equal-sized arrays laid end to
// end put the same voxel of every array on the same HBM channel and bank)
constexpr size_t TGV_SKEW = 69888;

// the early-stopping rule of tomo_pdtv_tol / tomo_roftv_tol (include/tomo_mi355x.h)
constexpr int TGV_TOL_INTERVAL = 6, TGV_TOL_MIN_SAVED = 3;

}  // namespace

// ------------------------------------------------------------------------------------------ C-ABI
extern "C" size_t tomo_tgv_scratch_bytes(int dx, int dy, int dz, int nd)
{
    if (nd == 2) dz = 1;
    const size_t narr = nd == 2 ? 10 : 16;   // U-bar, V, V-bar, P (nd each), Q (3 or 6)
    return narr * (tgv_align_up((size_t)dx * dy * dz * sizeof(float), 256) + TGV_SKEW);
}

extern "C" int tomo_tgv(int device, const float *in_dev, float *out_dev, int dx, int dy, int dz, int nd,
                        float lambda, float alpha1, float alpha0, float tau, float sigma, int iters,
                        double tol, int *iters_done, double *last_rel_change, void *stream)
{
    TOMO_REQUIRE(device >= 0, "The gpu_device must be a positive integer or zero");
    TOMO_REQUIRE(nd == 2 || nd == 3, "2D or 3D arrays must be provided only");
    if (nd == 2) dz = 1;
    TOMO_REQUIRE(dx >= 1 && dy >= 1 && dz >= 1, "TGV needs every dimension >= 1");
    TOMO_REQUIRE(iters >= 0, "TGV: the number of iterations must not be negative");
    TOMO_REQUIRE(lambda > 0.0f && alpha1 > 0.0f && alpha0 > 0.0f, "TGV: lambda, alpha1 and alpha0 must be positive");
    TOMO_REQUIRE(tau > 0.0f && sigma > 0.0f, "TGV: the step sizes tau and sigma must be positive");
    TOMO_REQUIRE(tol >= 0.0 && std::isfinite(tol), "the tolerance must be a finite number >= 0");
    TOMO_REQUIRE((size_t)dx * (size_t)dy < ((size_t)1 << 29), "a plane of %d x %d exceeds the 2 GiB a buffer descriptor of the TV kernels addresses", dx, dy);
    TOMO_REQUIRE(in_dev && out_dev, "NULL data pointer");
    TOMO_REQUIRE(in_dev != out_dev, "TGV: the output must not alias the input (U is iterated in the output array)");
    TOMO_ON_DEVICE(device);
    hipStream_t st = as_stream(stream);
    const size_t nvox = (size_t)dx * dy * dz;
    if (iters_done) *iters_done = iters;
    if (last_rel_change) *last_rel_change = NAN;
    TOMO_HIP(hipMemcpyAsync(out_dev, in_dev, nvox * sizeof(float), hipMemcpyDeviceToDevice, st));   // U = f
    if (iters == 0) return TOMO_OK;

    const size_t total = tomo_tgv_scratch_bytes(dx, dy, dz, nd);
    void *base = nullptr;
    int rc = tomo_arena_get(device, st, ARENA_TV, total, &base, true);
    if (rc != TOMO_OK) return rc;
    float *snap = nullptr;   // U_{n-6}: a block of its own, the TV arena keeps its size and placement
    if (tol > 0.0 && iters >= TGV_TOL_INTERVAL + TGV_TOL_MIN_SAVED) {
        void *p = nullptr;
        rc = tomo_arena_get(device, st, ARENA_TVSNAP, nvox * sizeof(float), &p);
        if (rc != TOMO_OK) return rc;
        snap = (float *)p;
    }

    const size_t step = tgv_align_up(nvox * sizeof(float), 256) + TGV_SKEW;
    char *cur = (char *)base;
    auto take = [&]() { float *p = (float *)cur; cur += step; return p; };
    TgvArgs a;
    a.f = in_dev; a.u = out_dev;
    a.ub = take();
    for (int c = 0; c < 3; ++c) a.v[c] = a.vb[c] = a.p[c] = nullptr;
    for (int k = 0; k < 6; ++k) a.q[k] = nullptr;
    for (int c = 0; c < nd; ++c) a.v[c] = take();
    for (int c = 0; c < nd; ++c) a.vb[c] = take();
    for (int c = 0; c < nd; ++c) a.p[c] = take();
    for (int k = 0; k < (nd == 3 ? 6 : 3); ++k) a.q[k] = take();
    a.dx = dx; a.dy = dy; a.dz = dz;
    a.lambda = lambda; a.alpha1 = alpha1; a.alpha0 = alpha0; a.tau = tau; a.sigma = sigma;
    // U-bar = f; V, V-bar, P, Q = 0 (one fill over the rest of the block, skews included)
    TOMO_HIP(hipMemcpyAsync(a.ub, in_dev, nvox * sizeof(float), hipMemcpyDeviceToDevice, st));
    TOMO_HIP(hipMemsetAsync(a.v[0], 0, total - step, st));

    for (int n = 1; n <= iters; ++n) {
        rc = tgv_launch_iteration(a, nd, st);
        if (rc != TOMO_OK) return rc;
        if (snap == nullptr || n % TGV_TOL_INTERVAL != 0 || iters - n < TGV_TOL_MIN_SAVED) continue;
        // the first check reads the caller's input as the reference and only writes the snapshot; later ones compare with
        // the snapshot and refresh it in the same pass
        double s[2];
        rc = tomo_rel_change(out_dev, n == TGV_TOL_INTERVAL ? in_dev : snap, snap, nvox, s, st);
        if (rc != TOMO_OK) return rc;
        const double d = s[0] == 0.0 ? 0.0 : (s[1] == 0.0 ? INFINITY : sqrt(s[0] / s[1]));
        if (last_rel_change) *last_rel_change = d;
        if (d < tol) {
            if (iters_done) *iters_done = n;
            return TOMO_OK;
        }
    }
    return TOMO_OK;
}
