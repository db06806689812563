// What the two back projectors share: the voxel-driven one (proj_kernels.hip, bp_brick.inl) and the matched one
// (bp_matched.hip).  The argument struct, the per-voxel arithmetic of the fused epilogues -- stated once, here -- and the host
// front end of the eight tomo_bp3d* entry points.  The load / store wrappers around bp_value (bp_epilogue*, mb_epilogue*) stay
// with their kernels: they decide a kernel's memory traffic, and the measured traffic profiles are keyed to those files.
// Internal linkage throughout, like the kernels that take a BpArgs.
#pragma once
#include "tomo_common.h"

namespace {

typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));

template <bool LERP8>
__device__ __forceinline__ float lerp_w(float f, float fl)
{
    float w = f - fl;
    if (LERP8) w = rintf(w * 256.0f) * (1.0f / 256.0f);
    return w;
}

enum { EPI_PLAIN = 0, EPI_FISTA = 1, EPI_FISTA_MOM = 2, EPI_ADMM = 3 };

struct BpArgs {
    const float *sino;       // [nz][na][nu]; zquad: [ceil(nz/4)][na][nu][4] (TOMO_RESIDUAL_ZQUAD, fused epilogues only)
    int zquad;               // (voxel-driven kernels only)
    const tomo_angle_t *tab; // na records
    int nz, n, nu, na;
    float *vol;              // EPI_PLAIN: output volume
    // fused epilogues
    const float *xt;         // FISTA: X_t (in)         ADMM: x
    int xt_zquad;            // EPI_FISTA, brick kernel only: xt is [ceil(nz/4)][n][n][4] (TOMO_VOLUME_ZQUAD, see tomo_mi355x.h)
    float *xout;             // FISTA: X (out)          ADMM: z (in/out)
    float *xt_out;           // FISTA_MOM: new X_t      ADMM: zu (out)
    const float *xold;       // FISTA_MOM: X_old (==xout buffer)   ADMM: u
    float s0, s1, s2, s3;    // FISTA: l_inv, beta ; ADMM: tau, rho, (1-alpha), alpha
    int nonneg, relax_on;
    int ntx, nty, nzb;       // tile counts
    int epi_aligned;         // every array the epilogue touches is 16-byte aligned (the dwordx4 epilogues)
    int device;              // host side only: the context's device (made current around the launch)
    std::string *path;       // host side only: receives the name of the kernel that ran
};

// One voxel of an epilogue: gradient g and the values read -> the (up to) two values written.  No contraction: these are
// the separate CuPy ufunc roundings of methodsIR_CuPy.py:463-475,545-557, and every back-projection kernel gets them from here.
//   PLAIN                                     -> o0 = g
//   FISTA      i0 = X_t                       -> o0 = X
//   FISTA_MOM  i0 = X_t, i1 = X_old           -> o0 = X, o1 = new X_t
//   ADMM       i0 = z, i1 = u, i2 = x         -> o0 = z, o1 = z + u
template <int EPI>
__device__ __forceinline__ void bp_value(const BpArgs &a, float g, float i0, float i1, float i2, float &o0, float &o1)
{
    if (EPI == EPI_PLAIN) {
        o0 = g;
    } else if (EPI == EPI_FISTA || EPI == EPI_FISTA_MOM) {
        float x = i0 - a.s0 * g;
        if (a.nonneg) x = x < 0.0f ? 0.0f : x;
        o0 = x;
        if (EPI == EPI_FISTA_MOM) o1 = x + a.s1 * (x - i1);
    } else {
        const float ga = a.s1 * ((i0 - i2) + i1);
        float z = i0 - a.s0 * (g + ga);
        if (a.nonneg) z = z < 0.0f ? 0.0f : z;
        if (a.relax_on) z = a.s2 * i0 + a.s3 * z;
        o0 = z;
        o1 = z + i1;
    }
}

// ------------------------------------------------------------------------------------------ host front end
// An entry point is: bp_prepare, the filler of its fused form, its kernel's own refusals, its kernel's launch.
int bp_prepare(tomo_ctx *ctx, int subset, const float *sino, BpArgs &a)
{
    TOMO_REQUIRE(ctx != nullptr, "ctx is NULL");
    TOMO_REQUIRE(subset < ctx->os, "subset %d out of range (OS_number %d)", subset, ctx->os);
    const tomo_subset &s = *find_subset(ctx, subset);
    TOMO_REQUIRE(sino != nullptr || s.size == 0, "NULL sinogram pointer");
    a = BpArgs();
    a.device = ctx->device;
    a.path = &ctx->last_bp_path;
    a.sino = sino;
    a.tab = ctx->dev_table + s.table_offset;
    a.nz = ctx->nz; a.n = ctx->n; a.nu = ctx->nu; a.na = s.size;
    return TOMO_OK;
}

int bp_fill_plain(BpArgs &a, float *vol)
{
    TOMO_REQUIRE(vol != nullptr, "NULL volume pointer");
    a.vol = vol;
    return TOMO_OK;
}

int bp_fill_fista(BpArgs &a, const float *xt, float *xout, float l_inv, int nonneg)
{
    TOMO_REQUIRE(xt && xout, "NULL volume pointer");
    a.xt = xt; a.xout = xout; a.s0 = l_inv; a.nonneg = nonneg;
    return TOMO_OK;
}

int bp_fill_fista_momentum(BpArgs &a, float *xt, float *xold_x, float l_inv, float beta, int nonneg)
{
    TOMO_REQUIRE(xt && xold_x, "NULL volume pointer");
    a.xt = xt; a.xt_out = xt; a.xold = xold_x; a.xout = xold_x;
    a.s0 = l_inv; a.s1 = beta; a.nonneg = nonneg;
    return TOMO_OK;
}

int bp_fill_admm(BpArgs &a, float *z, const float *x, const float *u, float *zu_out, float tau, float rho, int relax_on,
                 float one_minus_alpha, float alpha, int nonneg)
{
    TOMO_REQUIRE(z && x && u && zu_out, "NULL volume pointer");
    a.xt = x; a.xout = z; a.xt_out = zu_out; a.xold = u;
    a.s0 = tau; a.s1 = rho; a.s2 = one_minus_alpha; a.s3 = alpha;
    a.nonneg = nonneg; a.relax_on = relax_on;
    return TOMO_OK;
}

// is every array the epilogue EPI touches 16-byte aligned?
template <int EPI>
int bp_epi_aligned(const BpArgs &a)
{
    uintptr_t bits = 0;
    if (EPI == EPI_PLAIN) bits |= (uintptr_t)a.vol;
    else bits |= (uintptr_t)a.xt | (uintptr_t)a.xout;
    if (EPI == EPI_FISTA_MOM || EPI == EPI_ADMM) bits |= (uintptr_t)a.xt_out | (uintptr_t)a.xold;
    return (bits & 15) == 0;
}

}  // namespace
