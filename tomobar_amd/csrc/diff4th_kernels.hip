// Diff4th regulariser for gfx950: anisotropic fourth-order diffusion (Hajiaboli), explicit in time,
//     U' = U - tau (lambda Lap(W) + (U - f)),   U^0 = f,
// with W = cw^2 U_nn + cw U_tt the second derivatives along and across the gradient weighted by cw = 1 / (1 + |grad U|^2 /
// sigma^2).  The reference's dicts_check names Diff4th next to time_marching_step (tomobar/supp/dicts.py:173, "ROF_TV,
// LLT_ROF, NDF, Diff4th") but nothing in its tree implements it: what is computed is the algorithm stated in
// docs/kernels/diff4th.md, formula-level parity, unpinned -- tests/_diff4th_oracle.py restates it in numpy and the kernel
// reproduces its float32 form bit for bit (one rounding per operation in the stated order, no FMA contraction:
// -ffp-contract=off and no fmaf here; / is the compiler's correctly rounded division).
//
// One launch per iteration with both stages fused, a plane march on the skeleton of ndf_zmarch.inl (diff4th_zmarch.inl): W
// stays in registers, U is read once (plus halos and the seam planes of a z-chunk), f read once, U' written once -- 12 B
// per voxel and iteration.  The launch reads neighbours of the field it writes, so U is ping-ponged between the caller's
// output array and ONE work array in the placed TV arena; the first iteration reads the input itself as U^0 and the last
// one writes the output array.  The same kernel serves the z-slab form (tomo_diff4th_iter_slab_range): arrays with two
// ghost planes per interior boundary.
//
// The wave shifts, the plane I/O, the z-march grid, the array skew, the tolerance rule and the host driver of the time march
// are the one copy in zmarch_common.h, shared with tgv_kernels.hip, ndf_kernels.hip and llt_rof_kernels.hip.
// tv_kernels.hip keeps a copy of its own: it is pinned by hash (profiles/pmc_traffic.json), so it cannot include the header.
#include "zmarch_common.h"

namespace {

// One iteration on arrays of `planes` planes [dy][dx]: the output planes [out_begin, out_end) of `u_out` are written.  A
// plane of the arrays has a z-neighbour wherever the arrays hold one: the whole volume is planes = dz, a z-slab carries
// its ghost planes inside `planes` (the z index is clamped only at the global faces).
struct D4Args {
    const float *f;      // the input (read at the output voxels only)
    const float *u_in;   // the current iterate (the input itself in the first iteration)
    float *u_out;
    int dx, dy, planes, out_begin, out_end;
    float lambda, sigma, tau;
};

#include "diff4th_zmarch.inl"

// The only Diff4th launch site: 8 rows per lane, 2 x 2 waves (docs/kernels/diff4th.md, "Choosing RY").
static int d4_launch_iteration(const D4Args &a, int nd, hipStream_t st)
{
    const int rc = nd == 3 ? d4_zmarch_launch<3, 8, 2, 2>(a, st) : d4_zmarch_launch<2, 8, 2, 2>(a, st);
    if (rc != TOMO_OK) return rc;
    TOMO_LAUNCH_CHECK();
    return TOMO_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------ C-ABI
extern "C" size_t tomo_diff4th_scratch_bytes(int dx, int dy, int dz, int nd) { return march_scratch_bytes(dx, dy, dz, nd); }

extern "C" int tomo_diff4th(int device, const float *in_dev, float *out_dev, int dx, int dy, int dz, int nd,
                            float lambda, float sigma, float tau, int iters,
                            double tol, int *iters_done, double *last_rel_change, void *stream)
{
    TOMO_REQUIRE(lambda > 0.0f && sigma > 0.0f && tau > 0.0f, "Diff4th: lambda, the edge threshold sigma and the step tau must be positive");
    const int planes = nd == 2 ? 1 : dz;
    D4Args a{in_dev, nullptr, nullptr, dx, dy, planes, 0, planes, lambda, sigma, tau};
    return march_run("Diff4th", device, in_dev, out_dev, dx, dy, dz, nd, iters, tol, iters_done, last_rel_change, stream,
                     [&](const float *u_in, float *u_out) {
                         a.u_in = u_in; a.u_out = u_out;
                         return d4_launch_iteration(a, nd, as_stream(stream));
                     });
}

extern "C" int tomo_diff4th_iter_slab_range(int device, const float *in_dev, const float *u_in_dev, float *u_out_dev,
                                            int dx, int dy, int nz_local, int lo_planes, int hi_planes, int z_begin,
                                            int z_end, float lambda, float sigma, float tau, void *stream)
{
    TOMO_REQUIRE(lambda > 0.0f && sigma > 0.0f && tau > 0.0f, "Diff4th: lambda, the edge threshold sigma and the step tau must be positive");
    const D4Args a{in_dev, u_in_dev, u_out_dev, dx, dy, lo_planes + nz_local + hi_planes, lo_planes + z_begin, lo_planes + z_end,
                   lambda, sigma, tau};
    return march_slab_range("Diff4th", 2, device, in_dev, u_in_dev, u_out_dev, dx, dy, nz_local, lo_planes, hi_planes, z_begin, z_end,
                            [&] { return d4_launch_iteration(a, 3, as_stream(stream)); });
}
