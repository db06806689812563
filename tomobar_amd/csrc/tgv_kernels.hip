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
// The wave shifts, the plane I/O, the z-march grid, the array skew and the tolerance rule are the one copy in
// zmarch_common.h, shared with ndf_kernels.hip, diff4th_kernels.hip and llt_rof_kernels.hip.
// tv_kernels.hip keeps a copy of its own: it is pinned by hash (profiles/pmc_traffic.json), so it cannot include the header.
#include "zmarch_common.h"

namespace {

// Q components; 2D uses the first three
enum { TQ11 = 0, TQ22 = 1, TQ12 = 2, TQ33 = 3, TQ13 = 4, TQ23 = 5 };

struct TgvArgs {
    const float *f;   // the input
    float *u, *ub;    // U (the caller's output array), U-bar
    float *v[3], *vb[3], *p[3], *q[6];
    int dx, dy, dz;
    float lambda, alpha1, alpha0, tau, sigma;
};

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

}  // namespace

// ------------------------------------------------------------------------------------------ C-ABI
extern "C" size_t tomo_tgv_scratch_bytes(int dx, int dy, int dz, int nd)
{
    if (nd == 2) dz = 1;
    const size_t narr = nd == 2 ? 10 : 16;   // U-bar, V, V-bar, P (nd each), Q (3 or 6)
    return narr * work_array_bytes((size_t)dx * dy * dz);
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
    float *snap;
    rc = tol_snapshot(device, st, tol, iters, nvox, snap);
    if (rc != TOMO_OK) return rc;

    const size_t step = work_array_bytes(nvox);
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
        if (!tol_due(snap, n, iters)) continue;
        TolCheck c;
        rc = tol_check(c, n, out_dev, in_dev, snap, nvox, tol, st);
        if (rc != TOMO_OK) return rc;
        if (last_rel_change) *last_rel_change = c.d;
        if (c.stop) {
            if (iters_done) *iters_done = n;
            return TOMO_OK;
        }
    }
    return TOMO_OK;
}
