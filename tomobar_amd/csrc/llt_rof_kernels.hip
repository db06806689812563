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
// The wave shifts, the plane I/O, the z-march grid, the array skew, the tolerance rule and the host driver of the time march
// are the one copy in zmarch_common.h, shared with tgv_kernels.hip, ndf_kernels.hip and diff4th_kernels.hip.
// tv_kernels.hip keeps a copy of its own: it is pinned by hash (profiles/pmc_traffic.json), so it cannot include the header.
#include "zmarch_common.h"

namespace {

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

#include "llt_rof_zmarch.inl"

// The only LLT_ROF launch site: 8 rows per lane, 2 x 2 waves (docs/kernels/llt_rof.md, "Choosing RY").
static int lr_launch_iteration(const LrArgs &a, int nd, hipStream_t st)
{
    const int rc = nd == 3 ? lr_zmarch_launch<3, 8, 2, 2>(a, st) : lr_zmarch_launch<2, 8, 2, 2>(a, st);
    if (rc != TOMO_OK) return rc;
    TOMO_LAUNCH_CHECK();
    return TOMO_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------ C-ABI
extern "C" size_t tomo_llt_rof_scratch_bytes(int dx, int dy, int dz, int nd) { return march_scratch_bytes(dx, dy, dz, nd); }

extern "C" int tomo_llt_rof(int device, const float *in_dev, float *out_dev, int dx, int dy, int dz, int nd,
                            float lambda_rof, float lambda_llt, float tau, int iters,
                            double tol, int *iters_done, double *last_rel_change, void *stream)
{
    TOMO_REQUIRE(lambda_rof > 0.0f && lambda_llt > 0.0f && tau > 0.0f, "LLT_ROF: the ROF weight, the LLT weight and the step tau must be positive");
    const int planes = nd == 2 ? 1 : dz;
    LrArgs a{in_dev, nullptr, nullptr, dx, dy, planes, 0, planes, lambda_rof, lambda_llt, tau};
    return march_run("LLT_ROF", device, in_dev, out_dev, dx, dy, dz, nd, iters, tol, iters_done, last_rel_change, stream,
                     [&](const float *u_in, float *u_out) {
                         a.u_in = u_in; a.u_out = u_out;
                         return lr_launch_iteration(a, nd, as_stream(stream));
                     });
}

extern "C" int tomo_llt_rof_iter_slab_range(int device, const float *in_dev, const float *u_in_dev, float *u_out_dev,
                                            int dx, int dy, int nz_local, int lo_planes, int hi_planes, int z_begin,
                                            int z_end, float lambda_rof, float lambda_llt, float tau, void *stream)
{
    TOMO_REQUIRE(lambda_rof > 0.0f && lambda_llt > 0.0f && tau > 0.0f, "LLT_ROF: the ROF weight, the LLT weight and the step tau must be positive");
    const LrArgs a{in_dev, u_in_dev, u_out_dev, dx, dy, lo_planes + nz_local + hi_planes, lo_planes + z_begin, lo_planes + z_end,
                   lambda_rof, lambda_llt, tau};
    return march_slab_range("LLT_ROF", 2, device, in_dev, u_in_dev, u_out_dev, dx, dy, nz_local, lo_planes, hi_planes, z_begin, z_end,
                            [&] { return lr_launch_iteration(a, 3, as_stream(stream)); });
}
