// Nonlinear diffusion (NDF) regulariser for gfx950: explicit time marching of
//     U' = U + tau (lambda sum_d [g(U[i + e_d] - U[i]) + g(U[i - e_d] - U[i])] - (U - f)),   U^0 = f,
// with the flux g chosen by a penalty: Huber (TV-like), Perona-Malik (edge sharpening) or Tukey biweight (edges above the
// threshold sigma are left alone).  The reference's dicts_check still names NDF next to time_marching_step
// (tomobar/supp/dicts.py:173, "ROF_TV, LLT_ROF, NDF, Diff4th") but nothing in its tree implements it: what is computed is the
// algorithm stated in docs/kernels/ndf.md, formula-level parity, unpinned -- tests/_ndf_oracle.py restates it in numpy and
// the kernel reproduces its float32 form bit for bit (one rounding per operation in the stated order, no FMA contraction:
// -ffp-contract=off and no fmaf here; / is the compiler's correctly rounded division).
//
// One launch per iteration, a plane march on the skeleton of rof_zmarch.inl / tgv_*.inl (ndf_zmarch.inl): U is read once
// (plus halos and the two seam planes of a z-chunk), f read once, U' written once -- 12 B per voxel and iteration.  The
// launch reads neighbours of the field it writes, so U is ping-ponged between the caller's output array and ONE work array
// in the placed TV arena; the first iteration reads the input itself as U^0 and the last one writes the output array.
// The same kernel serves the z-slab form (tomo_ndf_iter_slab_range): arrays with one ghost plane per interior boundary.
//
// The wave shifts, the plane I/O, the z-march grid, the array skew, the tolerance rule and the host driver of the time march
// are the one copy in zmarch_common.h, shared with tgv_kernels.hip, diff4th_kernels.hip and llt_rof_kernels.hip.
// tv_kernels.hip keeps a copy of its own: it is pinned by hash (profiles/pmc_traffic.json), so it cannot include the header.
#include "zmarch_common.h"

namespace {

enum { NDF_HUBER = 0, NDF_PM = 1, NDF_TUKEY = 2 };   // TOMO_NDF_* of include/tomo_mi355x.h

// One iteration on arrays of `planes` planes [dy][dx]: the output planes [out_begin, out_end) of `u_out` are written.  A
// plane of the arrays has a z-neighbour wherever the arrays hold one: the whole volume is planes = dz, a z-slab carries
// its ghost planes inside `planes` (the z differences are zero only at the global faces).
struct NdfArgs {
    const float *f;      // the input (read at the lane's own voxels only)
    const float *u_in;   // the current iterate (the input itself in the first iteration)
    float *u_out;
    int dx, dy, planes, out_begin, out_end;
    float lambda, sigma, tau;
};

#include "ndf_zmarch.inl"

// The only NDF launch site: 8 rows per lane, 2 x 2 waves (ROF_TV's shape: the same traffic).
static int ndf_launch_iteration(const NdfArgs &a, int nd, int penalty, hipStream_t st)
{
    int rc;
    if (nd == 3) {
        rc = penalty == NDF_HUBER ? ndf_zmarch_launch<3, NDF_HUBER, 8, 2, 2>(a, st)
           : penalty == NDF_PM    ? ndf_zmarch_launch<3, NDF_PM, 8, 2, 2>(a, st)
                                  : ndf_zmarch_launch<3, NDF_TUKEY, 8, 2, 2>(a, st);
    } else {
        rc = penalty == NDF_HUBER ? ndf_zmarch_launch<2, NDF_HUBER, 8, 2, 2>(a, st)
           : penalty == NDF_PM    ? ndf_zmarch_launch<2, NDF_PM, 8, 2, 2>(a, st)
                                  : ndf_zmarch_launch<2, NDF_TUKEY, 8, 2, 2>(a, st);
    }
    if (rc != TOMO_OK) return rc;
    TOMO_LAUNCH_CHECK();
    return TOMO_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------ C-ABI
extern "C" size_t tomo_ndf_scratch_bytes(int dx, int dy, int dz, int nd) { return march_scratch_bytes(dx, dy, dz, nd); }

static int ndf_check(float lambda, float sigma, float tau, int penalty)
{
    TOMO_REQUIRE(lambda > 0.0f && sigma > 0.0f && tau > 0.0f, "NDF: lambda, the edge threshold sigma and the step tau must be positive");
    TOMO_REQUIRE(penalty == NDF_HUBER || penalty == NDF_PM || penalty == NDF_TUKEY, "NDF: the penalty must be 0 (Huber), 1 (PM) or 2 (Tukey)");
    return TOMO_OK;
}

extern "C" int tomo_ndf(int device, const float *in_dev, float *out_dev, int dx, int dy, int dz, int nd,
                        float lambda, float sigma, float tau, int penalty, int iters,
                        double tol, int *iters_done, double *last_rel_change, void *stream)
{
    if (int rc = ndf_check(lambda, sigma, tau, penalty)) return rc;
    const int planes = nd == 2 ? 1 : dz;
    NdfArgs a{in_dev, nullptr, nullptr, dx, dy, planes, 0, planes, lambda, sigma, tau};
    return march_run("NDF", device, in_dev, out_dev, dx, dy, dz, nd, iters, tol, iters_done, last_rel_change, stream,
                     [&](const float *u_in, float *u_out) {
                         a.u_in = u_in; a.u_out = u_out;
                         return ndf_launch_iteration(a, nd, penalty, as_stream(stream));
                     });
}

extern "C" int tomo_ndf_iter_slab_range(int device, const float *in_dev, const float *u_in_dev, float *u_out_dev,
                                        int dx, int dy, int nz_local, int lo_planes, int hi_planes, int z_begin,
                                        int z_end, float lambda, float sigma, float tau, int penalty, void *stream)
{
    if (int rc = ndf_check(lambda, sigma, tau, penalty)) return rc;
    const NdfArgs a{in_dev, u_in_dev, u_out_dev, dx, dy, lo_planes + nz_local + hi_planes, lo_planes + z_begin, lo_planes + z_end,
                    lambda, sigma, tau};
    return march_slab_range("NDF", 1, device, in_dev, u_in_dev, u_out_dev, dx, dy, nz_local, lo_planes, hi_planes, z_begin, z_end,
                            [&] { return ndf_launch_iteration(a, 3, penalty, as_stream(stream)); });
}
